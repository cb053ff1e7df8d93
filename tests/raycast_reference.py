"""Numpy restatement of the ray-casting rules of include/nerf_hip.h ("ABI 7 additions.  Rays against a mesh"): R the hit rule, G the
triangle grid, V face visibility from a camera, S face selection.  Every rule comes twice: vectorised (what the GPU tests compare
with) and as plain loops over Python floats (the definition; IEEE doubles, one rounding per operation, nothing fused).  walk_model
is a scalar model of the interval walk of csrc/mesh_raycast.hip over a grid, which must equal brute force for every grid."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
INF = float("inf")
DBL_MAX = float(np.finfo(np.float64).max)
EPS = 2.0 ** -20
SKIP = 2.0 ** -40


def _mesh(v, f):
    return np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)


def face_part(v, f):
    """-> [F] bool: the faces that take part (indices in [0, V), nine finite coordinates)"""
    v, f = _mesh(v, f)
    ok = ((f >= 0) & (f < len(v))).all(1)
    fin = np.isfinite(v).all(1) if len(v) else np.zeros(0, bool)
    ok[ok] = fin[f[ok]].all(1)
    return ok


def ray_part(o, d):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def _corners(v, f, part):
    """-> A, B, C [F, 3] fp64 (0 for the faces that take no part), mn, mx [F, 3] = the boxes widened by e"""
    v, f = _mesh(v, f)
    fs = np.where(part[:, None], f, 0)
    P = v[fs].astype(F64) if len(v) else np.zeros((len(f), 3, 3))
    P[~part] = 0.0
    e = EPS * np.abs(P).max((1, 2)) if len(f) else np.zeros(0)
    return P[:, 0], P[:, 1], P[:, 2], P.min(1) - e[:, None], P.max(1) + e[:, None]


def _cross(a, b):
    return (a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])


# ---- R: the hit rule ----

def cast(v, f, o, d, tmin=0.0, tmax=INF, skip=None, chunk=64):
    """Brute force over all faces -> (t [N] fp64, uv [N, 2] fp64, face [N] int32, side [N] int8)"""
    v, f = _mesh(v, f)
    o32, d32 = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    N, F = len(o32), len(f)
    t_out, uv, face, side = np.full(N, INF), np.zeros((N, 2)), np.full(N, -1, np.int32), np.zeros(N, np.int8)
    if N == 0 or F == 0:
        return t_out, uv, face, side
    part = face_part(v, f)
    A, B, C, mn, mx = _corners(v, f, part)
    e1, e2 = B - A, C - A
    rp = ray_part(o32, d32)
    skip = None if skip is None else np.asarray(skip, np.int64).reshape(N)
    fid = np.arange(F)
    tmin, tmax = F64(tmin), F64(tmax)
    with np.errstate(all="ignore"):
        for r0 in range(0, N, chunk):
            sl = slice(r0, min(N, r0 + chunk))
            oo, dd = o32[sl].astype(F64)[:, None, :], d32[sl].astype(F64)[:, None, :]
            oo, dd = np.where(rp[sl, None, None], oo, 0.0), np.where(rp[sl, None, None], dd, 0.0)
            px, py, pz = _cross(dd, e2[None])
            det = (e1[None, :, 0] * px + e1[None, :, 1] * py) + e1[None, :, 2] * pz
            s = oo - A[None]
            qx, qy, qz = _cross(s, e1[None])
            u = ((s[..., 0] * px + s[..., 1] * py) + s[..., 2] * pz) / det
            w = ((dd[..., 0] * qx + dd[..., 1] * qy) + dd[..., 2] * qz) / det
            t = ((e2[None, :, 0] * qx + e2[None, :, 1] * qy) + e2[None, :, 2] * qz) / det
            ok = part[None] & rp[sl, None] & (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (tmin <= t) & (t <= tmax)
            for k in range(3):
                h = oo[..., k] + t * dd[..., k]
                ok &= (mn[None, :, k] <= h) & (h <= mx[None, :, k])
            if skip is not None:
                ok &= fid[None] != skip[sl, None]
            tt = np.where(ok, t, INF)
            best = tt.min(1)
            first = (ok & (tt == best[:, None])).argmax(1)  # the lowest index among the ties
            hit = ok.any(1)
            rows = np.arange(len(best))
            t_out[sl] = np.where(hit, t[rows, first], INF)  # (that face's own t: -0.0 and 0.0 tie)
            uv[sl, 0] = np.where(hit, u[rows, first], 0.0)
            uv[sl, 1] = np.where(hit, w[rows, first], 0.0)
            face[sl] = np.where(hit, first, -1)
            side[sl] = np.where(hit, np.where(det[rows, first] > 0, 1, -1), 0)
    return t_out, uv, face, side


def _face_loop(v, f, i):
    """-> the nine coordinates [[ax, ay, az], ...] as Python floats, or None for a face that takes no part"""
    idx = [int(x) for x in f[i]]
    if any(x < 0 or x >= len(v) for x in idx):
        return None
    P = [[float(v[x][k]) for k in range(3)] for x in idx]
    return P if all(math.isfinite(c) for p in P for c in p) else None


def hit_loop(P, o, d, tmin, tmax):
    """The rule for one face (nine floats) and one ray (Python floats) -> (t, u, v, side) or None"""
    A, B, C = P
    e1 = [B[k] - A[k] for k in range(3)]
    e2 = [C[k] - A[k] for k in range(3)]
    p = [d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]]
    det = (e1[0] * p[0] + e1[1] * p[1]) + e1[2] * p[2]
    if not det != 0.0:
        return None
    s = [o[k] - A[k] for k in range(3)]
    q = [s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]]
    with np.errstate(all="ignore"):
        u = float(F64((s[0] * p[0] + s[1] * p[1]) + s[2] * p[2]) / F64(det))
        w = float(F64((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]) / F64(det))
        t = float(F64((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2]) / F64(det))
        if not (u >= 0.0 and w >= 0.0 and u + w <= 1.0 and tmin <= t <= tmax):
            return None
        e = EPS * max(abs(c) for c in A + B + C)
        for k in range(3):
            h = float(F64(o[k]) + F64(t) * F64(d[k]))
            if not (min(A[k], B[k], C[k]) - e <= h <= max(A[k], B[k], C[k]) + e):
                return None
    return t, u, w, (1 if det > 0.0 else -1)


def cast_loops(v, f, o, d, tmin=0.0, tmax=INF, skip=None):
    """cast() as plain loops"""
    v, f = _mesh(v, f)
    o32, d32 = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    N = len(o32)
    t_out, uv, face, side = np.full(N, INF), np.zeros((N, 2)), np.full(N, -1, np.int32), np.zeros(N, np.int8)
    Ps = [_face_loop(v, f, i) for i in range(len(f))]
    for i in range(N):
        oo, dd = [float(x) for x in o32[i]], [float(x) for x in d32[i]]
        if not all(math.isfinite(x) for x in oo + dd) or not any(x != 0.0 for x in dd):
            continue
        best = None
        for j in range(len(f)):
            if Ps[j] is None or (skip is not None and int(skip[i]) == j):
                continue
            r = hit_loop(Ps[j], oo, dd, float(tmin), float(tmax))
            if r is not None and (best is None or r[0] < best[0][0] or (r[0] == best[0][0] and j < best[1])):
                best = (r, j)
        if best is not None:
            (t_out[i], uv[i, 0], uv[i, 1], side[i]), face[i] = best[0], best[1]
    return t_out, uv, face, side


# ---- G: the triangle grid ----

def cellidx(x, lo, cell):
    with np.errstate(all="ignore"):
        return np.floor((np.asarray(x, F64) - F64(F32(lo))) / F64(F32(cell)))


def grid_boxes(v, f, lo, cell, dims):
    """-> (part [F], inside [F], b0 [F, 3], b1 [F, 3] float index boxes)"""
    part = face_part(v, f)
    _, _, _, mn, mx = _corners(v, f, part)
    lo = np.asarray(lo, F32).reshape(3)
    b0 = np.stack([cellidx(mn[:, k], lo[k], cell) for k in range(3)], 1) if len(part) else np.zeros((0, 3))
    b1 = np.stack([cellidx(mx[:, k], lo[k], cell) for k in range(3)], 1) if len(part) else np.zeros((0, 3))
    top = np.asarray(dims, F64).reshape(3) - 1
    inside = part & (b0 >= 0).all(1) & (b1 <= top).all(1)
    return part, inside, b0, b1


def grid_counts(v, f, lo, cell, dims):
    """-> [faces that take part, entries E, OUTSIDE faces]"""
    part, inside, b0, b1 = grid_boxes(v, f, lo, cell, dims)
    E = int(np.prod((b1 - b0 + 1)[inside], axis=1).sum()) if inside.any() else 0
    return [int(part.sum()), E, int((part & ~inside).sum())]


def grid_counts_loops(v, f, lo, cell, dims):
    v, f = _mesh(v, f)
    n = [0, 0, 0]
    for i in range(len(f)):
        P = _face_loop(v, f, i)
        if P is None:
            continue
        n[0] += 1
        e = EPS * max(abs(c) for p in P for c in p)
        vol, inside = 1, True
        for k in range(3):
            a = math.floor(((min(p[k] for p in P) - e) - float(F32(lo[k]))) / float(F32(cell)))
            b = math.floor(((max(p[k] for p in P) + e) - float(F32(lo[k]))) / float(F32(cell)))
            inside = inside and a >= 0 and b <= dims[k] - 1
            vol *= b - a + 1
        if inside:
            n[1] += vol
        else:
            n[2] += 1
    return n


def point_grid_rule(lo, hi, m):
    """The sizing rule of the nearest-point grid (include/nerf_hip.h C.2), restated"""
    lo = np.asarray(lo, F32).reshape(3)
    ext = np.asarray(hi, F32).reshape(3).astype(F64) - lo.astype(F64)
    pos = ext > 0
    if m <= 0 or not pos.any():
        return lo, F32(1.0), (1, 1, 1)
    with np.errstate(all="ignore"):
        cell = F32((np.prod(ext[pos]) / m) ** (1.0 / int(pos.sum())))
    if not cell >= F32(2.0 ** -126):
        cell = F32(2.0 ** -126)
    cell = min(cell, F32(2.0 ** 127))
    while True:
        dims = tuple(int(np.floor(e / F64(cell))) + 1 if e > 0 else 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= 2 * m + 8:
            return lo, F32(cell), dims
        if cell >= F32(2.0 ** 127):
            return lo, F32(cell), (1, 1, 1)
        cell = F32(cell * F32(2.0))


def raycast_grid(v, f):
    """The sizing rule of the triangle grid: the point rule over the finite vertices' box grown by 2^-19 of its largest |coordinate|,
    with m = F, the cell doubled while E > 4 F + 64"""
    v, f = _mesh(v, f)
    fin = np.isfinite(v).all(1)
    if not fin.any():
        return np.zeros(3, F32), F32(1.0), (1, 1, 1)
    glo, ghi = v[fin].min(0), v[fin].max(0)
    pad = F32(2.0 ** -19) * F32(max(np.abs(glo).max(), np.abs(ghi).max()))
    glo, ghi = (glo - pad).astype(F32), (ghi + pad).astype(F32)
    lo, cell, dims = point_grid_rule(glo, ghi, len(f))
    ext = ghi.astype(F64) - glo.astype(F64)
    while grid_counts(v, f, lo, cell, dims)[1] > 4 * len(f) + 64 and cell < F32(2.0 ** 127):
        cell = F32(cell * F32(2.0))
        dims = tuple(int(np.floor(e / F64(cell))) + 1 if e > 0 else 1 for e in ext)
    return lo, cell, dims


def walk_model(v, f, grid, o, d, tmin=0.0, tmax=INF, skip=None, stats=None):
    """The interval walk of csrc/mesh_raycast.hip as scalar Python: the OUTSIDE faces in full, then per interval of t the entries of the
    cells between the two ends' cell indices.  Must equal cast() for EVERY grid.  stats (a dict): 'tests' counts the faces asked."""
    v, f = _mesh(v, f)
    lo, cell, dims = grid
    lo = [float(F32(x)) for x in np.asarray(lo).reshape(3)]
    cell = float(F32(cell))
    part, inside, b0, b1 = grid_boxes(v, f, lo, cell, dims)
    cells = {}
    for j in np.flatnonzero(inside):
        for x in range(int(b0[j, 0]), int(b1[j, 0]) + 1):
            for y in range(int(b0[j, 1]), int(b1[j, 1]) + 1):
                for z in range(int(b0[j, 2]), int(b1[j, 2]) + 1):
                    cells.setdefault((x, y, z), []).append(int(j))
    outside = [int(j) for j in np.flatnonzero(part & ~inside)]
    tlo, thi = max(float(tmin), -DBL_MAX), min(float(tmax), DBL_MAX)

    def cidx(t, oo, dd):
        with np.errstate(all="ignore"):
            return [float(np.floor((F64(oo[k]) + F64(t) * F64(dd[k]) - F64(lo[k])) / F64(cell))) for k in range(3)]

    def faces_of_ray(i, oo, dd):
        if not tlo <= thi:
            return
        yield from outside
        ad = [abs(x) for x in dd]
        m = (0 if ad[0] >= ad[2] else 2) if ad[0] >= ad[1] else (1 if ad[1] >= ad[2] else 2)
        om, dm, lom, nm = oo[m], dd[m], lo[m], float(dims[m])
        fwd = dm > 0.0
        tc = tlo
        with np.errstate(all="ignore"):
            plane = lom if fwd else lom + nm * cell
            te = float((F64(plane) - F64(om)) / F64(dm))
            ts = float((F64(te) - ((abs(om) + abs(plane)) * SKIP) / abs(dm)) - abs(F64(te)) * SKIP)
        if ts > tc:
            cs = cidx(ts, oo, dd)[m]
            if (cs < 0.0) if fwd else (cs > nm - 1.0):
                if ts >= thi:
                    return
                tc = ts
        cc = cidx(tc, oo, dd)
        if (cc[m] > nm - 1.0) if fwd else (cc[m] < 0.0):
            return
        j = int(min(max(cc[m], 0.0), nm - 1.0))
        prev = None
        for _ in range(int(nm) + 3):
            tn = thi
            if 0 <= j <= nm - 1:
                with np.errstate(all="ignore"):
                    tn = float((F64(lom + float(j + 1 if fwd else j) * cell) - F64(om)) / F64(dm))
                tn = min(max(tn, tc) if not math.isnan(tn) else tc, thi)
            cn = cidx(tn, oo, dd)
            box = []
            for k in range(3):
                a, b, top = min(cc[k], cn[k]), max(cc[k], cn[k]), dims[k] - 1.0
                box.append(None if b < 0.0 or a > top else (int(min(max(a, 0.0), top)), int(min(max(b, 0.0), top))))
            if None not in box:
                for x in range(box[0][0], box[0][1] + 1):
                    for y in range(box[1][0], box[1][1] + 1):
                        for z in range(box[2][0], box[2][1] + 1):
                            if prev is not None and all(prev[k][0] <= c <= prev[k][1] for k, c in enumerate((x, y, z))):
                                continue
                            yield from cells.get((x, y, z), ())
                prev = box
            else:
                prev = None
            stop = yield ("end", tn)
            if stop or tn >= thi or ((cn[m] > nm - 1.0) if fwd else (cn[m] < 0.0)):
                return
            tc, cc = tn, cn
            j += 1 if fwd else -1
        raise AssertionError("the walk did not end")

    # the generator protocol above keeps the model in one place; drive it with the best-so-far rule
    o32, d32 = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    N = len(o32)
    t_out, uv, face, side = np.full(N, INF), np.zeros((N, 2)), np.full(N, -1, np.int32), np.zeros(N, np.int8)
    Ps = [_face_loop(v, f, i) for i in range(len(f))]
    for i in range(N):
        oo, dd = [float(x) for x in o32[i]], [float(x) for x in d32[i]]
        if not all(math.isfinite(x) for x in oo + dd) or not any(x != 0.0 for x in dd):
            continue
        best = None
        gen = faces_of_ray(i, oo, dd)
        try:
            item = next(gen)
            while True:
                if isinstance(item, tuple):  # the end of an interval: stop when best < t_next, strictly
                    item = gen.send(best is not None and best[0][0] < item[1])
                    continue
                j = item
                if stats is not None:
                    stats["tests"] = stats.get("tests", 0) + 1
                if Ps[j] is not None and not (skip is not None and int(skip[i]) == j):
                    r = hit_loop(Ps[j], oo, dd, float(tmin), float(tmax))
                    if r is not None and (best is None or r[0] < best[0][0] or (r[0] == best[0][0] and j < best[1])):
                        best = (r, j)
                item = next(gen)
        except StopIteration:
            pass
        if best is not None:
            (t_out[i], uv[i, 0], uv[i, 1], side[i]), face[i] = best[0], best[1]
    return t_out, uv, face, side


# ---- V: face visibility ----

def camera_q(pose17, K_inv):
    """Q = inverse(R K^T) in fp64 and the camera's position (fp32) from one pose row [17] and K_inv [3, 3]"""
    pb = np.asarray(pose17, F32).reshape(17)
    R = pb[:15].reshape(3, 5)[:, :3].astype(F64)
    K = np.asarray(K_inv, F32).reshape(3, 3).astype(F64)
    return np.linalg.inv(R @ K.T), pb[:15].reshape(3, 5)[:, 3].copy()


def face_rays(v, f, cam, Q, H, W):
    """-> (orig [F, 3] fp32, dir [F, 3] fp32, valid [F] uint8)"""
    v, f = _mesh(v, f)
    part = face_part(v, f)
    A, B, C, _, _ = _corners(v, f, part)
    cam = np.asarray(cam, F32).reshape(3).astype(F64)
    Q = np.asarray(Q, F64).reshape(3, 3)
    with np.errstate(all="ignore"):
        G = ((A + B) + C) / 3.0
        nx, ny, nz = _cross(B - A, C - A)
        w = cam[None] - G
        facing = (nx * w[:, 0] + ny * w[:, 1]) + nz * w[:, 2] > 0
        a, b, c = -w[:, 0], -w[:, 1], -w[:, 2]
        m = [(Q[i, 0] * a + Q[i, 1] * b) + Q[i, 2] * c for i in range(3)]
        x, y = m[0] / m[2], m[1] / m[2]
        view = (m[2] > 0) & (-0.5 <= x) & (x < H - 0.5) & (-0.5 <= y) & (y < W - 0.5)
        valid = part & facing & view
        orig = np.where(part[:, None], G, 0.0).astype(F32)
        dirs = np.where(valid[:, None], cam[None] - orig.astype(F64), 0.0).astype(F32)
    return orig, dirs, valid.astype(np.uint8)


def face_rays_loops(v, f, cam, Q, H, W):
    v, f = _mesh(v, f)
    cam = [float(F32(x)) for x in np.asarray(cam).reshape(3)]
    Q = np.asarray(Q, F64).reshape(3, 3).tolist()
    orig, dirs, valid = np.zeros((len(f), 3), F32), np.zeros((len(f), 3), F32), np.zeros(len(f), np.uint8)
    for i in range(len(f)):
        P = _face_loop(v, f, i)
        if P is None:
            continue
        A, B, C = P
        G = [((A[k] + B[k]) + C[k]) / 3.0 for k in range(3)]
        e1, e2 = [B[k] - A[k] for k in range(3)], [C[k] - A[k] for k in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        w = [cam[k] - G[k] for k in range(3)]
        facing = (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2] > 0.0
        m = [(Q[r][0] * -w[0] + Q[r][1] * -w[1]) + Q[r][2] * -w[2] for r in range(3)]
        with np.errstate(all="ignore"):
            x, y = float(F64(m[0]) / F64(m[2])), float(F64(m[1]) / F64(m[2]))
            view = m[2] > 0.0 and -0.5 <= x < H - 0.5 and -0.5 <= y < W - 0.5
            orig[i] = np.asarray(G, F64).astype(F32)
        if facing and view:
            valid[i] = 1
            dirs[i] = np.asarray([cam[k] - float(orig[i, k]) for k in range(3)], F64).astype(F32)
    return orig, dirs, valid


def visibility(v, f, cams, H, W, tmin=1e-4):
    """cams: [(Q, cam_o)] as camera_q gives them -> (seen [F] bool, per-camera counts, valid [n, F])"""
    v, f = _mesh(v, f)
    seen, counts, valids = np.zeros(len(f), bool), [], []
    own = np.arange(len(f))
    for Q, cam in cams:
        orig, dirs, valid = face_rays(v, f, cam, Q, H, W)
        hit = cast(v, f, orig, dirs, tmin, 1.0, skip=own)[2] >= 0
        vis = (valid != 0) & ~hit
        seen |= vis
        counts.append(int(vis.sum()))
        valids.append(valid)
    return seen, counts, np.asarray(valids).reshape(len(cams), len(f))


# ---- S: face selection ----

def select_faces(v, f, keep, normals=None, rgb=None):
    """-> (verts, faces int32, normals, rgb): the kept faces and the vertices they use, both in their order"""
    v, f = _mesh(v, f)
    kept = (np.asarray(keep).reshape(-1) != 0) & ((f >= 0) & (f < len(v))).all(1)
    used = np.zeros(len(v), bool)
    used[f[kept].reshape(-1)] = True
    newidx = np.cumsum(used) - 1
    pick = lambda a: None if a is None else np.asarray(a, F32).reshape(-1, 3)[used]
    return v[used], newidx[f[kept]].astype(np.int32).reshape(-1, 3), pick(normals), pick(rgb)


def select_faces_loops(v, f, keep, normals=None, rgb=None):
    v, f = _mesh(v, f)
    kept = [i for i in range(len(f)) if keep[i] and all(0 <= int(x) < len(v) for x in f[i])]
    used = sorted({int(x) for i in kept for x in f[i]})
    new = {x: k for k, x in enumerate(used)}
    pick = lambda a: None if a is None else np.asarray([np.asarray(a, F32).reshape(-1, 3)[x] for x in used], F32).reshape(-1, 3)
    return pick(v), np.asarray([[new[int(x)] for x in f[i]] for i in kept], np.int32).reshape(-1, 3), pick(normals), pick(rgb)


# ---- fixtures ----

def unit_cube():
    """-> (verts [8, 3], faces [12, 3]): the cube [0, 1]^3, outward faces, each square split along the diagonal from its lowest corner"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def _box(v):
    v = np.asarray(v, F32).reshape(-1, 3)
    fin = v[np.isfinite(v).all(1) & (np.abs(v) < 1e6).all(1)]
    return (fin.min(0), fin.max(0)) if len(fin) else (np.zeros(3, F32), np.ones(3, F32))


def lattice_rays(v, step=1.5):
    """Rays down the three axes through lattice and half-lattice points of the unit lattice (multiples of 0.5, every `step`), from one
    unit before the mesh's box -> (o, d)"""
    lo, hi = _box(v)
    o, d = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        gb = np.arange(np.floor(lo[b]), np.ceil(hi[b]) + 0.25, step, dtype=F64)
        gc = np.arange(np.floor(lo[c]), np.ceil(hi[c]) + 0.25, step, dtype=F64)
        B, C = np.meshgrid(gb, gc, indexing="ij")
        p = np.zeros((B.size, 3))
        p[:, a], p[:, b], p[:, c] = np.floor(lo[a]) - 1.0, B.ravel(), C.ravel()
        q = np.zeros((B.size, 3))
        q[:, a] = 1.0
        o.append(p)
        d.append(q)
    return np.concatenate(o).astype(F32), np.concatenate(d).astype(F32)


def random_rays(v, n, seed, inside=None):
    """n rays towards random points of the mesh's box, from a shell around it or (inside) from one point within -> (o, d), d not normalised"""
    lo, hi = _box(v)
    rng = np.random.default_rng(seed)
    c, r = (lo + hi).astype(F64) / 2, float(np.linalg.norm((hi - lo).astype(F64))) / 2 + 1e-3
    target = lo + rng.random((n, 3)) * (hi - lo)
    if inside is not None:
        o = np.tile(np.asarray(inside, F64).reshape(1, 3), (n, 1))
    else:
        u = rng.normal(size=(n, 3))
        o = c + u / np.linalg.norm(u, axis=1, keepdims=True) * r * 1.5
    return o.astype(F32), (target - o).astype(F32)


def plane_rays(grid, n=6):
    """Origins exactly on cell planes of the grid (lo + k cell in fp32 on every axis), axis-aligned directions both ways -> (o, d)"""
    lo, cell, dims = grid
    lo = np.asarray(lo, F32).reshape(3)
    ks = [np.unique(np.linspace(0, dims[k], n).astype(int)) for k in range(3)]
    P = np.stack(np.meshgrid(*[(lo[k] + ks[k].astype(F32) * F32(cell)).astype(F32) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    o, d = [], []
    for a in range(3):
        for sgn in (1.0, -1.0):
            q = np.zeros_like(P)
            q[:, a] = sgn
            o.append(P)
            d.append(q)
    return np.concatenate(o).astype(F32), np.concatenate(d).astype(F32)


def bad_rays():
    """Rays that take no part (NaN, inf, d = 0) between two that do -> (o, d)"""
    nan, inf = np.nan, np.inf
    o = np.array([[-1, 8, 8], [nan, 8, 8], [-1, inf, 8], [-1, 8, 8], [-1, 8, 8], [-1, 8, -inf], [-1, 8, 8], [-1, 8, 8]], F32)
    d = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [1, nan, 0], [1, 0, 0], [inf, 0, 0], [1, 0.01, 0]], F32)
    return o, d


def nested_blobs():
    """blobs plus a copy of its second ball shrunk to half size about its own centre -> (verts, faces, inner [F] bool)"""
    import simplify_meshes as M

    v, f, _ = M.blobs()
    (c, r) = M.BALLS[1]
    c = np.asarray(c, F32)
    near = np.linalg.norm(v.astype(F64) - c.astype(F64), axis=1) < r + 1.5
    fsel = near[f].all(1)
    used = np.zeros(len(v), bool)
    used[f[fsel].reshape(-1)] = True
    new = np.cumsum(used) - 1
    vi = ((v[used] - c) * F32(0.5) + c).astype(F32)
    fi = (new[f[fsel]] + len(v)).astype(np.int32)
    inner = np.concatenate((np.zeros(len(f), bool), np.ones(len(fi), bool)))
    return np.concatenate((v, vi)), np.concatenate((f, fi)).astype(np.int32), inner
