"""numpy restatements of rules TC, S and M of include/nerf_hip.h (colour fusion beside the TSDF, the colour volume sampled at points,
marching cubes under a mask of valid lattice points): each once vectorised and once in scalar loops written
from the header's text, and the analytic colour images of tsdf_reference's sphere scene.  Builds on tsdf_reference.py and
mc_reference.py; nothing here needs a device."""
import functools

import numpy as np

import mc_reference as MC
import tsdf_reference as R

F32, F64 = np.float32, np.float64


# ---- rule TC ----

def integrate_color(T, Wt, C, lo, step, depth, opacity, rgb, cams, trunc, min_opacity=0.5, carve=True):
    """Rules T and TC, vectorised over the voxels: T, Wt fp32 [nx, ny, nz], C fp32 [nx, ny, nz, 4] (none modified), depth [n, H, W],
    opacity the same or None, rgb [n, H, W, 3], cams a list of (Q, cam_o) -> the new (T, Wt, C)."""
    T, Wt, C = np.array(T, F32), np.array(Wt, F32), np.array(C, F32)
    P = R.lattice(lo, step, T.shape).astype(F64)
    depth, rgb = np.asarray(depth, F32), np.asarray(rgb, F32)
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
            pix = rgb[c][xi, yi]  # [nx, ny, nz, 3]
            cobs = obs & (sdf <= trunc) & np.isfinite(pix).all(-1)
            val = np.minimum(1.0, sdf / trunc)
            if carve:
                bg = view & ~fg
                val = np.where(bg, 1.0, val)
                obs = obs | bg
            T64, W64 = T.astype(F64), Wt.astype(F64)
            T = np.where(obs, (((T64 * W64) + val) / (W64 + 1.0)).astype(F32), T)
            Wt = np.where(obs, (W64 + 1.0).astype(F32), Wt)
            C64 = C.astype(F64)
            wc = C64[..., 3]
            new = np.empty_like(C)
            for ch in range(3):
                new[..., ch] = (((C64[..., ch] * wc) + pix[..., ch].astype(F64)) / (wc + 1.0)).astype(F32)
            new[..., 3] = (wc + 1.0).astype(F32)
            C = np.where(cobs[..., None], new, C)
    return T, Wt, C


def integrate_color_loops(T, Wt, C, lo, step, depth, opacity, rgb, cams, trunc, min_opacity=0.5, carve=True):
    """Rules T and TC once more, one voxel and one view at a time in numpy scalars, written from the header's text alone."""
    T, Wt, C = np.array(T, F32), np.array(Wt, F32), np.array(C, F32)
    lo, step, depth, rgb = np.asarray(lo, F32), np.asarray(step, F32), np.asarray(depth, F32), np.asarray(rgb, F32)
    n, H, W = depth.shape
    trunc, one, half = F64(trunc), F64(1.0), F64(0.5)
    with np.errstate(all="ignore"):
        for i in range(T.shape[0]):
            for j in range(T.shape[1]):
                for k in range(T.shape[2]):
                    p = [F64(F32(lo[a] + F32(F32(q) * step[a]))) for a, q in enumerate((i, j, k))]
                    t, wt = T[i, j, k], Wt[i, j, k]
                    col = [C[i, j, k, ch] for ch in range(4)]
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
                            px = rgb[c, xi, yi]
                            if sdf <= trunc and np.isfinite(px[0]) and np.isfinite(px[1]) and np.isfinite(px[2]):
                                wc = F64(col[3])
                                col = [F32(((F64(col[ch]) * wc) + F64(px[ch])) / (wc + one)) for ch in range(3)] + [F32(wc + one)]
                        elif carve:
                            val = one
                        else:
                            continue
                        t = F32(((F64(t) * F64(wt)) + val) / (F64(wt) + one))
                        wt = F32(F64(wt) + one)
                    T[i, j, k], Wt[i, j, k] = t, wt
                    C[i, j, k] = col
    return T, Wt, C


# ---- rule S ----

def sample_color(C, lo, step, points):
    """Rule S, vectorised over the points: C fp32 [nx, ny, nz, 4], points [M, 3] fp32 -> (rgb [M, 3] fp32, valid [M] bool)."""
    C, pts = np.asarray(C, F32), np.asarray(points, F32).reshape(-1, 3)
    lo, step = np.asarray(lo, F32).astype(F64), np.asarray(step, F32).astype(F64)
    dims = C.shape[:3]
    M = len(pts)
    finite = np.isfinite(pts).all(1)
    x = np.where(finite[:, None], pts, F32(0)).astype(F64)
    i0, f = np.zeros((M, 3), np.int64), np.zeros((M, 3), F64)
    with np.errstate(all="ignore"):
        for a in range(3):
            if dims[a] > 1:
                g = (x[:, a] - lo[a]) / step[a]
                ci = np.minimum(np.maximum(np.floor(g), 0.0), F64(dims[a] - 2))
                i0[:, a] = ci.astype(np.int64)
                f[:, a] = np.minimum(np.maximum(g - ci, 0.0), 1.0)
        num, den = np.zeros((M, 3), F64), np.zeros(M, F64)
        for di in range(min(2, dims[0])):
            for dj in range(min(2, dims[1])):
                for dk in range(min(2, dims[2])):
                    c = C[i0[:, 0] + di, i0[:, 1] + dj, i0[:, 2] + dk].astype(F64)
                    has = finite & (c[:, 3] > 0)
                    wx = f[:, 0] if di else 1.0 - f[:, 0]
                    wy = f[:, 1] if dj else 1.0 - f[:, 1]
                    wz = f[:, 2] if dk else 1.0 - f[:, 2]
                    w = (wx * wy) * wz
                    num = np.where(has[:, None], num + w[:, None] * c[:, :3], num)
                    den = np.where(has, den + w, den)
        valid = den > 0
        rgb = np.where(valid[:, None], (num / np.where(valid, den, 1.0)[:, None]).astype(F32), F32(0)).astype(F32)
    return rgb, valid


def sample_color_loops(C, lo, step, points):
    """Rule S once more, one point at a time in numpy scalars."""
    C, pts = np.asarray(C, F32), np.asarray(points, F32).reshape(-1, 3)
    lo, step = np.asarray(lo, F32), np.asarray(step, F32)
    dims = C.shape[:3]
    rgb, valid = np.zeros((len(pts), 3), F32), np.zeros(len(pts), bool)
    zero, one = F64(0.0), F64(1.0)
    with np.errstate(all="ignore"):
        for m, x in enumerate(pts):
            if not (np.isfinite(x[0]) and np.isfinite(x[1]) and np.isfinite(x[2])):
                continue
            i0, f = [0, 0, 0], [zero, zero, zero]
            for a in range(3):
                if dims[a] > 1:
                    g = (F64(x[a]) - F64(lo[a])) / F64(step[a])
                    ci = min(max(np.floor(g), zero), F64(dims[a] - 2))
                    i0[a] = int(ci)
                    f[a] = min(max(g - ci, zero), one)
            num, den = [zero, zero, zero], zero
            for di in range(min(2, dims[0])):
                for dj in range(min(2, dims[1])):
                    for dk in range(min(2, dims[2])):
                        c = C[i0[0] + di, i0[1] + dj, i0[2] + dk]
                        if not c[3] > 0:
                            continue
                        w = ((f[0] if di else one - f[0]) * (f[1] if dj else one - f[1])) * (f[2] if dk else one - f[2])
                        num = [num[ch] + w * F64(c[ch]) for ch in range(3)]
                        den = den + w
            if den > 0:
                valid[m] = True
                rgb[m] = [F32(num[ch] / den) for ch in range(3)]
    return rgb, valid


# ---- rule M ----

def live_cells(valid):
    """[nx - 1, ny - 1, nz - 1] bool: the cells whose eight corners are valid"""
    v = np.asarray(valid) != 0
    nx, ny, nz = v.shape
    live = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for dx, dy, dz in MC.CORNERS:
        live &= v[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    return live


def face_cells(sigma, level, table=None):
    """the linear index (C order over the cells) of the cell each face of mc_reference.marching_cubes(sigma, level) comes from"""
    s = np.ascontiguousarray(sigma, F32)
    nx, ny, nz = s.shape
    table = MC.load_table() if table is None else table
    with np.errstate(all="ignore"):
        inside = s > F32(level)
    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(MC.CORNERS):
        cube |= (~inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]).astype(np.int64) << c
    nt = ((table >= 0).sum(axis=1) // 3)[cube.reshape(-1)]
    return np.repeat(np.arange(cube.size), nt)


def marching_cubes_masked(sigma, valid, level, lo=(0, 0, 0), step=(1, 1, 1), table=None):
    """Rule M, vectorised: the unmasked mesh of mc_reference restricted to the live cells -> (verts, faces, normals).  A vertex stays
    iff one of the up to four cells around its edge is live; survivors keep their order and are renumbered."""
    s = np.ascontiguousarray(sigma, F32)
    nx, ny, nz = s.shape
    verts, faces, normals = MC.marching_cubes(s, level, lo, step, table)
    if min(nx, ny, nz) < 2:
        return verts, faces, normals
    live = live_cells(valid)
    pad = np.zeros((nx + 1, ny + 1, nz + 1), bool)  # pad[i + 1, j + 1, k + 1] = live[i, j, k]; False outside
    pad[1:nx, 1:ny, 1:nz] = live
    around = np.zeros((nx, ny, nz, 3), bool)  # per lattice point and axis: a live cell contains the edge to the +axis neighbour
    for ax in range(3):
        for da in range(2):
            for db in range(2):
                off = [1, 1, 1]
                others = [a for a in range(3) if a != ax]
                off[others[0]] -= da
                off[others[1]] -= db
                around[..., ax] |= pad[off[0]:off[0] + nx, off[1]:off[1] + ny, off[2]:off[2] + nz]
    with np.errstate(all="ignore"):
        inside = s > F32(level)
    own = np.zeros((nx, ny, nz, 3), bool)
    own[:-1, :, :, 0] = inside[:-1] != inside[1:]
    own[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    own[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    keep_v = around[own]  # in the unmasked vertex order (row-major over point, axis)
    assert keep_v.size == len(verts)
    remap = np.where(keep_v, np.cumsum(keep_v) - 1, -1).astype(np.int32)
    keep_f = live.reshape(-1)[face_cells(s, level, table)]
    f = remap[faces[keep_f]]
    assert (f >= 0).all(), "a face of a live cell uses an edge without a vertex"
    return verts[keep_v], f.astype(np.int32).reshape(-1, 3), normals[keep_v]


def marching_cubes_masked_loops(sigma, valid, level, lo=(0, 0, 0), step=(1, 1, 1), table=None):
    """Rule M and the vertex, normal and face rules once more, one lattice point and one cell at a time in fp32 scalars."""
    s = np.ascontiguousarray(sigma, F32)
    v = np.asarray(valid) != 0
    dims = s.shape
    nx, ny, nz = dims
    level, lo, step = F32(level), np.asarray(lo, F32).reshape(3), np.asarray(step, F32).reshape(3)
    table = MC.load_table() if table is None else table
    if min(dims) < 2:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3), F32)

    def live(i, j, k):
        if min(i, j, k) < 0 or i + 1 >= nx or j + 1 >= ny or k + 1 >= nz:
            return False
        return all(v[i + dx, j + dy, k + dz] for dx, dy, dz in MC.CORNERS)

    def grad(q, a):
        lo_, hi_ = list(q), list(q)
        if q[a] == 0:
            hi_[a] += 1
            return F32(F32(s[tuple(hi_)] - s[tuple(q)]) / step[a])
        if q[a] == dims[a] - 1:
            lo_[a] -= 1
            return F32(F32(s[tuple(q)] - s[tuple(lo_)]) / step[a])
        lo_[a] -= 1
        hi_[a] += 1
        return F32(F32(s[tuple(hi_)] - s[tuple(lo_)]) / F32(F32(2) * step[a]))

    verts, normals, vid = [], [], {}
    with np.errstate(all="ignore"):
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    q = (i, j, k)
                    for ax in range(3):
                        b = list(q)
                        b[ax] += 1
                        if b[ax] >= dims[ax] or (s[q] > level) == (s[tuple(b)] > level):
                            continue
                        back = [a for a in range(3) if a != ax]
                        cells = []
                        for da in range(2):
                            for db in range(2):
                                c = list(q)
                                c[back[0]] -= da
                                c[back[1]] -= db
                                cells.append(live(*c))
                        if not any(cells):
                            continue
                        vid[(q, ax)] = len(verts)
                        s0, s1 = s[q], s[tuple(b)]
                        t = F32(F32(level - s0) / F32(s1 - s0))
                        if not np.isfinite(t):
                            t = F32(0.5)
                        pa = [F32(lo[a] + F32(F32(q[a]) * step[a])) for a in range(3)]
                        pb = F32(lo[ax] + F32(F32(q[ax] + 1) * step[ax]))
                        x = list(pa)
                        x[ax] = F32(pa[ax] + F32(t * F32(pb - pa[ax])))
                        g = []
                        for a in range(3):
                            ga, gb = grad(q, a), grad(tuple(b), a)
                            g.append(F32(ga + F32(t * F32(gb - ga))))
                        ln = F32(np.sqrt(F32(F32(F32(g[0] * g[0]) + F32(g[1] * g[1])) + F32(g[2] * g[2]))))
                        ok = np.isfinite(ln) and ln > 0
                        verts.append(x)
                        normals.append([F32(-g[a] / ln) if ok else F32(0) for a in range(3)])
        faces = []
        for i in range(nx - 1):
            for j in range(ny - 1):
                for k in range(nz - 1):
                    if not live(i, j, k):
                        continue
                    row = MC.cube_index([s[i + dx, j + dy, k + dz] > level for dx, dy, dz in MC.CORNERS])
                    tri = [e for e in table[row] if e >= 0]
                    for t0 in range(0, len(tri), 3):
                        f = []
                        for e in tri[t0:t0 + 3]:
                            o = MC.EDGE_OWNER[e]
                            f.append(vid[((i + int(o[0]), j + int(o[1]), k + int(o[2])), int(MC.EDGE_AXIS[e]))])
                        faces.append(f)
    return (np.asarray(verts, F32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3))


# ---- the scenes ----

def sphere_colors(pose17, K, H, W, radius=R.SPHERE_R):
    """[H, W, 3] fp32: 0.5 + 0.5 * hit / |hit| where the pixel's unit ray meets the sphere, 0 where it misses"""
    o, u = R.unit_rays(pose17, K, H, W)
    b = u @ o
    disc = b * b - (o @ o - radius * radius)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    hit = o + t[..., None] * u
    col = 0.5 + 0.5 * hit / np.linalg.norm(hit, axis=-1, keepdims=True)
    return np.where((disc > 0)[..., None], col, 0.0).astype(F32)


@functools.lru_cache(maxsize=None)
def sphere_rgb():
    """the colour images [8, H, W, 3] of tsdf_reference.sphere_scene() (computed once; read-only)"""
    s = R.sphere_scene()
    out = np.stack([sphere_colors(p, s["K"], s["H"], s["W"]) for p in s["poses"]])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sphere_fused_color(carve=True):
    """the restatement's (T, Wt, C) of the sphere scene with sphere_rgb() from zero (computed once per carve; read-only)"""
    s = R.sphere_scene()
    z = np.zeros(s["shape"], F32)
    out = integrate_color(z, z, np.zeros(s["shape"] + (4,), F32), s["lo"], s["step"], s["depth"], s["opacity"], sphere_rgb(), s["cams"], s["trunc"],
                          0.5, carve)
    for a in out:
        a.setflags(write=False)
    return out


def random_rgb(s, seed=5, bad=True):
    """random colour images [n, H, W, 3] for a tsdf_reference case, with (bad) some NaN and inf channels"""
    rng = np.random.default_rng(seed)
    rgb = rng.random(s["depth"].shape + (3,)).astype(F32)
    if bad:
        u = rng.random(rgb.shape)
        rgb[u < 0.03] = np.nan
        rgb[(u >= 0.03) & (u < 0.05)] = np.inf
        rgb[(u >= 0.05) & (u < 0.06)] = -np.inf
    return rgb


def random_color_volume(shape, seed=7, empty=0.4):
    """a random colour volume [nx, ny, nz, 4] with about ``empty`` of the Wc zero"""
    rng = np.random.default_rng(seed)
    C = rng.random(tuple(shape) + (4,)).astype(F32)
    C[..., 3] = np.where(rng.random(shape) < empty, 0.0, rng.integers(1, 9, shape)).astype(F32)
    return C


def random_grid_and_mask(shape, seed=11, valid=0.95):
    """a random grid in [-1, 1) with a NaN or two, and a random mask with about ``valid`` of the points valid"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1.0, 1.0, shape).astype(F32)
    g.reshape(-1)[rng.integers(0, g.size, 2)] = np.nan
    return g, (rng.random(shape) < valid)
