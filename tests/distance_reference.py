"""numpy restatement of the geometry evaluation (include/nerf_hip.h "ABI 7 additions"): measure() /
sample_surface() / nearest() / distance_stats() / chamfer() vectorised, the *_loops functions a plain-loop reading of the same header
text (tests/test_mesh_distance_cpu.py holds one against the other), nearest_brute the O(N M) definition, and the point clouds only
these tests use.  int64 sums wrap like the device's two's complement (np.add on int64); Python ints where the text says int64 and a
check of the range matters."""
import functools

import numpy as np

import smooth_reference as S

F32 = np.float32
ONE = float(2 ** 40)
W_ONE = float(2 ** 39)
D_ONE = float(2 ** 30)
M32 = 0xFFFFFFFF


# ---- A. measures ----

def _faces(verts, faces, lo, scale):
    """-> (part [F] bool, u [F, 3 corners, 3 axes] fp64 box coordinates (0 where the face takes no part), p [F, 3, 3] fp64 originals)"""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    uc, fin = S.box_coords(v, lo, scale)
    inr = ((f >= 0) & (f < V)).all(1)
    part = inr & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    fs = np.where(part[:, None], f, 0)
    if V:
        part &= fin[fs].all(1)
    fs = np.where(part[:, None], f, 0)
    if V == 0:
        return part, np.zeros((len(f), 3, 3)), np.zeros((len(f), 3, 3))
    u = np.where(part[:, None, None], uc[fs], 0.0)
    p = np.where(part[:, None, None], v[fs].astype(np.float64), 0.0)
    return part, u, p


def _cross_len(u):
    e1, e2 = u[:, 1] - u[:, 0], u[:, 2] - u[:, 0]
    N = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), axis=1)
    return np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])


def measure_raw(verts, faces, lo=None, scale=None):
    """-> the device's eight int64s as a list of Python ints (wrapped to int64)"""
    lo, scale = S.default_box(verts, lo, scale)
    part, u, _ = _faces(verts, faces, lo, scale)
    area = _cross_len(u) * 0.5
    a, b, c = u[:, 0], u[:, 1], u[:, 2]
    X = np.stack((b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]), axis=1)
    six = (a[:, 0] * X[:, 0] + a[:, 1] * X[:, 1]) + a[:, 2] * X[:, 2]
    mom = area[:, None] * (((a + b) + c) / 3.0)
    terms = np.concatenate((area[:, None], six[:, None], mom), axis=1)
    t = np.where(part[:, None], np.rint(terms * ONE), 0.0).astype(np.int64)
    with np.errstate(over="ignore"):
        sums = t.sum(0, dtype=np.int64)
    return [int(x) for x in sums] + [int(part.sum()), 0, 0]


def _uc_loop(v, i, d, lo, sc):
    return min(max((np.float64(v[i, d]) - np.float64(lo[d])) / sc, -1.0), 2.0)


def _face_loop(v, face):
    V = len(v)
    return (all(0 <= i < V for i in face) and len(set(face)) == 3 and all(bool(np.isfinite(v[i]).all()) for i in face))


def _wrap64(x):
    return (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def measure_loops(verts, faces, lo, scale):
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    lo = np.asarray(lo, F32).reshape(3)
    sc = np.float64(F32(scale))
    out = [0] * 8
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        if not _face_loop(v, face):
            continue
        ua, ub, uc = ([_uc_loop(v, i, d, lo, sc) for d in range(3)] for i in face)
        e1 = [ub[d] - ua[d] for d in range(3)]
        e2 = [uc[d] - ua[d] for d in range(3)]
        N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        length = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
        area = length * 0.5
        X = (ub[1] * uc[2] - ub[2] * uc[1], ub[2] * uc[0] - ub[0] * uc[2], ub[0] * uc[1] - ub[1] * uc[0])
        six = (ua[0] * X[0] + ua[1] * X[1]) + ua[2] * X[2]
        out[0] += int(np.rint(area * ONE))
        out[1] += int(np.rint(six * ONE))
        for d in range(3):
            out[2 + d] += int(np.rint((area * (((ua[d] + ub[d]) + uc[d]) / 3.0)) * ONE))
        out[5] += 1
    return [_wrap64(x) for x in out]


# ---- B. surface samples ----

def _fin(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def uniform(seed, i, stream):
    """r_stream of samples i (an array) -> fp64 in (0, 1)"""
    i = np.asarray(i, dtype=np.uint64)
    seed = np.uint64(int(seed) & M32)
    first = _fin(np.full(1, (int(seed) + 0x9E3779B9 * (stream + 1)) & M32, np.uint64))[0]
    h = _fin((_fin(first ^ i) + seed) & M32)
    return (h.astype(np.float64) + 0.5) / 4294967296.0


def _fin_loop(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def uniform_loop(seed, i, stream):
    seed &= M32
    h = _fin_loop((_fin_loop(_fin_loop((seed + 0x9E3779B9 * (stream + 1)) & M32) ^ i) + seed) & M32)
    return (np.float64(h) + 0.5) / 4294967296.0


def weights(verts, faces, lo=None, scale=None):
    """-> w [F] int64"""
    lo, scale = S.default_box(verts, lo, scale)
    part, u, _ = _faces(verts, faces, lo, scale)
    return np.where(part, np.rint(_cross_len(u) * W_ONE), 0.0).astype(np.int64)


def sample_surface(verts, faces, n, seed=0, lo=None, scale=None):
    """-> (points [n, 3] fp32, face [n] int32, W)"""
    lo, scale = S.default_box(verts, lo, scale)
    part, _, p = _faces(verts, faces, lo, scale)
    with np.errstate(over="ignore"):
        cum = np.cumsum(weights(verts, faces, lo, scale), dtype=np.int64)
    W = int(cum[-1]) if len(cum) else 0
    pts, face = np.zeros((n, 3), F32), np.full(n, -1, np.int32)
    if W <= 0 or n == 0:
        return pts, face, W
    i = np.arange(n, dtype=np.int64)
    x = np.floor(((i.astype(np.float64) + uniform(seed, i, 0)) / np.float64(n)) * np.float64(W))
    with np.errstate(invalid="ignore"):
        t = np.where(x >= 2.0 ** 63, W - 1, x.astype(np.int64))
    t = np.minimum(t, W - 1)
    f = np.minimum(np.searchsorted(cum, t, side="right"), len(cum) - 1)
    ok = part[f]
    r1, r2 = uniform(seed, i, 1), uniform(seed, i, 2)
    fold = r1 + r2 > 1.0
    r1, r2 = np.where(fold, 1.0 - r1, r1), np.where(fold, 1.0 - r2, r2)
    A, B, C = p[f, 0], p[f, 1], p[f, 2]
    with np.errstate(over="ignore"):
        q = ((A + r1[:, None] * (B - A)) + r2[:, None] * (C - A)).astype(F32)
    pts[ok] = q[ok]
    face[ok] = f[ok]
    return pts, face, W


def sample_loops(verts, faces, n, seed, lo, scale):
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    lo = np.asarray(lo, F32).reshape(3)
    sc = np.float64(F32(scale))
    flist = np.asarray(faces).reshape(-1, 3).tolist()
    cum, run = [], 0
    for face in flist:
        w = 0
        if _face_loop(v, face):
            ua, ub, uc = ([_uc_loop(v, i, d, lo, sc) for d in range(3)] for i in face)
            e1 = [ub[d] - ua[d] for d in range(3)]
            e2 = [uc[d] - ua[d] for d in range(3)]
            N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
            w = int(np.rint(np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]) * W_ONE))
        run += w
        cum.append(run)
    W = run
    assert W < 2 ** 63
    pts, fid = np.zeros((n, 3), F32), np.full(n, -1, np.int32)
    if W <= 0:
        return pts, fid, W
    for i in range(n):
        t = min(int(np.floor(((np.float64(i) + uniform_loop(seed, i, 0)) / np.float64(n)) * np.float64(W))), W - 1)
        f = next(k for k in range(len(cum)) if cum[k] > t)
        r1, r2 = uniform_loop(seed, i, 1), uniform_loop(seed, i, 2)
        if r1 + r2 > 1.0:
            r1, r2 = 1.0 - r1, 1.0 - r2
        a, b, c = (v[k].astype(np.float64) for k in flist[f])
        pts[i] = [F32((a[d] + r1 * (b[d] - a[d])) + r2 * (c[d] - a[d])) for d in range(3)]
        fid[i] = f
    return pts, fid, W


# ---- C. nearest points ----

def nearest_brute(ref, query, chunk=256):
    """The definition, O(N M): -> (idx [N] int32, dist2 [N] fp64)"""
    r = np.asarray(ref, dtype=F32).reshape(-1, 3)
    q = np.asarray(query, dtype=F32).reshape(-1, 3)
    keep = np.flatnonzero(np.isfinite(r).all(1))
    r64 = r[keep].astype(np.float64)
    idx, d2 = np.full(len(q), -1, np.int32), np.full(len(q), np.inf)
    qfin = np.isfinite(q).all(1)
    if len(keep) == 0:
        return idx, d2
    for s in range(0, len(q), chunk):
        sel = np.flatnonzero(qfin[s:s + chunk]) + s
        if len(sel) == 0:
            continue
        d = q[sel].astype(np.float64)[:, None, :] - r64[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        k = dd.argmin(1)  # (the first minimum: the lowest index, keep being ascending)
        idx[sel], d2[sel] = keep[k], dd[np.arange(len(sel)), k]
    return idx, d2


def nearest_loops(ref, query):
    r = np.asarray(ref, dtype=F32).reshape(-1, 3)
    q = np.asarray(query, dtype=F32).reshape(-1, 3)
    idx, d2 = np.full(len(q), -1, np.int32), np.full(len(q), np.inf)
    for j in range(len(q)):
        if not np.isfinite(q[j]).all():
            continue
        for i in range(len(r)):
            if not np.isfinite(r[i]).all():
                continue
            dx, dy, dz = (np.float64(q[j, d]) - np.float64(r[i, d]) for d in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            if d < d2[j]:  # (strictly: a later index never replaces an equal distance)
                idx[j], d2[j] = i, d
    return idx, d2


def nearest(ref, query):
    """The restatement the device is held against: a k-d tree has no place here -- the definition IS the brute force."""
    return nearest_brute(ref, query)


# ---- D. distance statistics ----

def distance_stats(dist2, unit, thresholds=()):
    """-> the device's 4 + K int64s as Python ints"""
    d2 = np.asarray(dist2, dtype=np.float64).reshape(-1)
    unit = np.float64(unit)
    ok = np.isfinite(d2) & (d2 >= 0)
    x = d2[ok]
    d, e = np.sqrt(x) / unit, x / (unit * unit)
    out = [int(ok.sum()), int(np.rint(np.minimum(d, 8.0) * D_ONE).astype(np.int64).sum()),
           int(np.rint(np.minimum(e, 64.0) * D_ONE).astype(np.int64).sum()), int(((d > 8.0) | (e > 64.0)).sum())]
    return out + [int((x <= np.float64(t) * np.float64(t)).sum()) for t in thresholds]


def distance_stats_loops(dist2, unit, thresholds=()):
    unit = np.float64(unit)
    out = [0] * (4 + len(thresholds))
    for x in np.asarray(dist2, dtype=np.float64).reshape(-1):
        if not np.isfinite(x) or not x >= 0:
            continue
        d, e = np.sqrt(x) / unit, x / (unit * unit)
        out[0] += 1
        out[1] += int(np.rint(min(d, 8.0) * D_ONE))
        out[2] += int(np.rint(min(e, 64.0) * D_ONE))
        out[3] += 1 if (d > 8.0 or e > 64.0) else 0
        for k, t in enumerate(thresholds):
            out[4 + k] += 1 if x <= np.float64(t) * np.float64(t) else 0
    return out


def default_unit(a, b):
    pts = [np.asarray(p, F32).reshape(-1, 3) for p in (a, b)]
    pts = [p[np.isfinite(p).all(1)] for p in pts]
    pts = [p for p in pts if len(p)]
    if not pts:
        return float(S.pow2_at_least(1.0))
    lo, hi = np.min([p.min(0) for p in pts], axis=0), np.max([p.max(0) for p in pts], axis=0)
    with np.errstate(all="ignore"):
        return float(S.pow2_at_least((hi - lo).astype(F32).max()))


def chamfer(a, b, thresholds=(), unit=None):
    """-> dict(raw_ab, raw_ba, unit, precision, recall, mean_ab, mean_ba): mesh.chamfer's ints and what it derives from them"""
    unit = default_unit(a, b) if unit is None else float(unit)
    _, d_ab = nearest(b, a)
    _, d_ba = nearest(a, b)
    ab, ba = distance_stats(d_ab, unit, thresholds), distance_stats(d_ba, unit, thresholds)
    frac = lambda raw, n: [w / n if n else float("nan") for w in raw[4:]]
    mean = lambda raw: raw[1] / (raw[0] * D_ONE) * unit if raw[0] else float("nan")
    return dict(raw_ab=ab, raw_ba=ba, unit=unit, precision=frac(ab, len(d_ab)), recall=frac(ba, len(d_ba)), mean_ab=mean(ab), mean_ba=mean(ba),
                d_ab=d_ab, d_ba=d_ba)


# ---- clouds and meshes of these tests ----

@functools.lru_cache(maxsize=None)
def cloud(n, seed, spread=1.0):
    p = (np.random.default_rng(seed).random((n, 3), dtype=F32) * F32(spread)).astype(F32)
    p.setflags(write=False)
    return p


def unit_cube():
    """-> (verts, faces): the cube [0, 1]^3, 12 outward triangles"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return v, f


def square(z, n=1):
    """-> (verts, faces): the unit square [0, 1]^2 at height z as 2 n^2 triangles"""
    g = np.linspace(0.0, 1.0, n + 1)
    v = np.array([[x, y, z] for x in g for y in g], F32)
    idx = lambda i, j: i * (n + 1) + j
    f = np.array([t for i in range(n) for j in range(n)
                  for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))], np.int32)
    return v, f
