"""numpy restatement of the edge topology, the smoothing steps and the face-derived vertex normals (include/nerf_hip.h, DESIGN.md
section 3h-6): topology() / step() / smooth() / vertex_normals() vectorised (np.unique on keys, np.add.at on int64), the *_loops
functions a plain-loop reading of the same definitions (tests/test_mesh_smooth_cpu.py holds one against the other), the default box of
mesh.smooth, and the meshes only the smoothing tests use."""
import functools

import numpy as np

F32 = np.float32
POS_ONE = float(2 ** 30)
NRM_ONE = float(2 ** 40)


# ---- the box ----

def pow2_at_least(ext):
    ext = F32(ext)
    if not ext > 0:
        return F32(1.0)
    if not np.isfinite(ext):
        return F32(2.0 ** 127)
    p = F32(2.0 ** -149)
    while p < ext and p < F32(2.0 ** 127):  # (every power of two of fp32, ascending)
        p = F32(p * F32(2.0))
    return p


def default_box(verts, lo=None, scale=None):
    """mesh.smooth_box: lo = the minimum over the finite vertices (unless given), scale = pow2_at_least(max over the axes of
    fp32(hi - lo)) (unless given); without a finite vertex lo = 0 and scale = 1 (unless given)."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    ok = np.isfinite(v).all(1)
    if not ok.any():
        return (np.zeros(3, F32) if lo is None else np.asarray(lo, F32).reshape(3)), F32(1.0 if scale is None else scale)
    lo = v[ok].min(0) if lo is None else np.asarray(lo, F32).reshape(3)
    if scale is None:
        with np.errstate(all="ignore"):
            scale = pow2_at_least((v[ok].max(0) - lo).astype(F32).max())
    return lo.astype(F32), F32(scale)


def box_coords(verts, lo, scale):
    """-> (uc [V, 3] fp64 clamped box coordinates -- 0 in the rows of vertices that are not finite --, finite [V] bool)"""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    fin = np.isfinite(v).all(1)
    with np.errstate(all="ignore"):
        u = (v.astype(np.float64) - np.asarray(lo, F32).astype(np.float64)) / np.float64(F32(scale))
    uc = np.where(fin[:, None], np.clip(u, -1.0, 2.0), 0.0)
    return uc, fin


# ---- A. edges and topology ----

def topology(faces, V):
    """-> dict(part [F] bool, ea / eb [E] int64 the edges' smaller / larger index in ascending key order, count, tally [E], degree,
    vert_flags [V] int32, counts = the device's eight: faces, edges, boundary, non-manifold, inconsistent, used vertices, 0, largest
    degree; euler, closed)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    part = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    fp = f[part]
    a, b = fp.reshape(-1), fp[:, [1, 2, 0]].reshape(-1)  # every face runs a -> b
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    count = np.zeros(len(uk), np.int64)
    tally = np.zeros(len(uk), np.int64)
    np.add.at(count, inv, 1)
    np.add.at(tally, inv, np.where(a < b, 1, -1))
    ea, eb = uk >> 32, uk & 0xFFFFFFFF
    degree = np.zeros(V, np.int64)
    np.add.at(degree, ea, 1)
    np.add.at(degree, eb, 1)
    flags = np.zeros(V, np.int64)
    for bit, sel in ((1, count == 1), (2, count > 2)):
        on = np.zeros(V, bool)
        on[ea[sel]] = True
        on[eb[sel]] = True
        flags |= np.where(on, bit, 0)
    nb, nm, ni = int((count == 1).sum()), int((count > 2).sum()), int(((count == 2) & (tally != 0)).sum())
    used = int((degree > 0).sum())
    counts = [int(part.sum()), len(uk), nb, nm, ni, used, 0, int(degree.max()) if V else 0]
    return dict(part=part, ea=ea, eb=eb, count=count, tally=tally, degree=degree.astype(np.int32), vert_flags=flags.astype(np.int32),
                counts=counts, euler=used - len(uk) + counts[0], closed=bool(counts[0] > 0 and nb == 0 and nm == 0 and ni == 0))


def topology_loops(faces, V):
    """The definition read one face at a time -> (degree, vert_flags, counts)"""
    count, tally = {}, {}
    n_part = 0
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        if any(not 0 <= i < V for i in face) or len(set(face)) < 3:
            continue
        n_part += 1
        for k in range(3):
            p, q = face[k], face[(k + 1) % 3]
            e = (min(p, q), max(p, q))
            count[e] = count.get(e, 0) + 1
            tally[e] = tally.get(e, 0) + (1 if p < q else -1)
    nbrs = [set() for _ in range(V)]
    flags = [0] * V
    for (p, q), c in count.items():
        nbrs[p].add(q)
        nbrs[q].add(p)
        for i in (p, q):
            flags[i] |= (1 if c == 1 else 0) | (2 if c > 2 else 0)
    degree = [len(s) for s in nbrs]
    counts = [n_part, len(count), sum(c == 1 for c in count.values()), sum(c > 2 for c in count.values()),
              sum(c == 2 and tally[e] != 0 for e, c in count.items()), sum(d > 0 for d in degree), 0, max(degree, default=0)]
    return np.asarray(degree, np.int32), np.asarray(flags, np.int32), counts


# ---- C. steps ----

def step(verts, topo, lo, scale, w, fix_boundary=True):
    """One step with weight w over topology()'s edges -> verts_out [V, 3] fp32"""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    V = len(v)
    lo64, sc64 = np.asarray(lo, F32).reshape(3).astype(np.float64), np.float64(F32(scale))
    uc, fin = box_coords(v, lo, scale)
    q = np.rint(uc * POS_ONE).astype(np.int64)
    S = np.zeros((V, 3), np.int64)
    n = np.zeros(V, np.int64)
    for src, dst in ((topo["ea"], topo["eb"]), (topo["eb"], topo["ea"])):
        m = fin[src]
        np.add.at(S, dst[m], q[src[m]])
        np.add.at(n, dst[m], 1)
    move = fin & (n > 0)
    if fix_boundary:
        move &= (topo["vert_flags"] & 1) == 0
    out = v.copy()
    with np.errstate(all="ignore"):
        p = v.astype(np.float64)
        mean = lo64 + sc64 * (S.astype(np.float64) / (n.astype(np.float64) * POS_ONE)[:, None])
        new = (p + np.float64(w) * (mean - p)).astype(F32)
    out[move] = new[move]
    return out


def step_loops(verts, faces, lo, scale, w, fix_boundary=True):
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    V = len(v)
    nbrs = [set() for _ in range(V)]
    count = {}
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        if any(not 0 <= i < V for i in face) or len(set(face)) < 3:
            continue
        for k in range(3):
            p, q = face[k], face[(k + 1) % 3]
            nbrs[p].add(q)
            nbrs[q].add(p)
            e = (min(p, q), max(p, q))
            count[e] = count.get(e, 0) + 1
    boundary = {i for e, c in count.items() if c == 1 for i in e}
    lo = np.asarray(lo, F32).reshape(3)
    sc = np.float64(F32(scale))
    out = v.copy()
    fin = lambda i: bool(np.isfinite(v[i]).all())
    for i in range(V):
        good = [j for j in nbrs[i] if fin(j)]
        if not fin(i) or not good or (fix_boundary and i in boundary):
            continue
        for d in range(3):
            S = 0
            for j in good:
                uc = min(max((np.float64(v[j, d]) - np.float64(lo[d])) / sc, -1.0), 2.0)
                S += int(np.rint(uc * POS_ONE))
            m = np.float64(lo[d]) + sc * (np.float64(S) / (np.float64(len(good)) * POS_ONE))
            p = np.float64(v[i, d])
            out[i, d] = F32(p + np.float64(w) * (m - p))
    return out


def smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, lo=None, scale=None):
    """mesh.smooth -> dict(verts, normals, topo, pinned, steps, lo, scale)"""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    lo, scale = default_box(v, lo, scale)
    topo = topology(faces, len(v))
    weights = ([lam] if mu is None else [lam, mu]) * int(iterations)
    cur = v
    for w in weights:
        cur = step(cur, topo, lo, scale, w, fix_boundary)
    return dict(verts=cur, normals=vertex_normals(cur, faces, lo, scale), topo=topo,
                pinned=int((topo["vert_flags"] & 1).sum()) if fix_boundary else 0, steps=len(weights), lo=lo, scale=scale)


# ---- D. normals ----

def normal_sums(verts, faces, lo, scale):
    """-> T [V, 3] int64 (wrapping like the device's two's-complement sums)"""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    V = len(v)
    uc, fin = box_coords(v, lo, scale)
    topo_part = topology(faces, V)["part"]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[topo_part]
    f = f[fin[f].all(1)] if len(f) else f
    T = np.zeros((V, 3), np.int64)
    if len(f):
        ua, ub, uc_ = uc[f[:, 0]], uc[f[:, 1]], uc[f[:, 2]]
        e1, e2 = ub - ua, uc_ - ua
        N = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), axis=1)
        term = np.rint(N * NRM_ONE).astype(np.int64)
        with np.errstate(over="ignore"):
            for c in range(3):
                np.add.at(T, f[:, c], term)
    return T


def normalise(T):
    t = T.astype(np.float64)
    length = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])[:, None]
    return np.where(length > 0, t / np.where(length > 0, length, 1.0), 0.0).astype(F32).reshape(-1, 3)


def vertex_normals(verts, faces, lo=None, scale=None):
    lo, scale = default_box(verts, lo, scale)
    return normalise(normal_sums(verts, faces, lo, scale))


def vertex_normals_loops(verts, faces, lo, scale):
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    V = len(v)
    lo = np.asarray(lo, F32).reshape(3)
    sc = np.float64(F32(scale))
    T = [[0, 0, 0] for _ in range(V)]
    for face in np.asarray(faces).reshape(-1, 3).tolist():
        if any(not 0 <= i < V for i in face) or len(set(face)) < 3 or not all(np.isfinite(v[i]).all() for i in face):
            continue
        u = [[min(max((np.float64(v[i, d]) - np.float64(lo[d])) / sc, -1.0), 2.0) for d in range(3)] for i in face]
        e1 = [u[1][d] - u[0][d] for d in range(3)]
        e2 = [u[2][d] - u[0][d] for d in range(3)]
        N = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        for i in face:
            for d in range(3):
                T[i][d] += int(np.rint(N[d] * NRM_ONE))
    out = np.zeros((V, 3), F32)
    for i in range(V):
        t = [np.float64(x) for x in T[i]]
        length = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        if length > 0:
            out[i] = [F32(x / length) for x in t]
    return out


# ---- measures and meshes of the smoothing tests ----

def volume(verts, faces):
    """The signed volume a closed, outward-oriented mesh encloses (fp64)"""
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


@functools.lru_cache(maxsize=None)
def sphere32():
    """-> (verts, faces, normals): the 32^3 field 11.3 - |x - (15.4, 15.7, 15.2)| at level 0"""
    import mc_reference as MC

    g = np.arange(32, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    s = 11.3 - np.sqrt((X - 15.4) ** 2 + (Y - 15.7) ** 2 + (Z - 15.2) ** 2)
    out = MC.marching_cubes(s.astype(np.float32), 0.0, (0, 0, 0), (1, 1, 1))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hub(n=5000):
    """One vertex joined to a ring of n: a disc fan of n faces, the hub slightly above the ring's plane.  -> (verts, faces)"""
    t = np.arange(n) * (2 * np.pi / n)
    r = 1.0 + 0.1 * np.sin(7 * t)
    v = np.concatenate((np.stack((r * np.cos(t), r * np.sin(t), 0.05 * np.cos(3 * t)), axis=1), [[0.013, -0.021, 0.4]])).astype(F32)
    i = np.arange(n)
    f = np.stack((np.full(n, n), i, (i + 1) % n), axis=1).astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def book(n=3000):
    """n faces around ONE edge (0, 1), every other one reversed: one key takes the inserts of more than one workgroup, in both
    directions; its ends have degree n + 1.  -> (verts, faces)"""
    t = np.arange(n) * (2 * np.pi / n)
    v = np.concatenate(([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5]], np.stack((np.cos(t), np.sin(t), 0.2 * np.sin(5 * t)), axis=1))).astype(F32)
    f = np.stack((np.zeros(n, np.int64), np.ones(n, np.int64), np.arange(n) + 2), axis=1)
    f[1::2] = f[1::2, ::-1]
    f = f.astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def patchwork():
    """A mesh of a few dozen faces with everything the definitions single out: an open 4 x 4 grid (a boundary), a fin on one of its
    interior edges (a non-manifold edge), one quad whose second triangle is flipped (a same-direction pair), a face with a repeated
    index, faces with indices -1, V and 2^31 - 1, a NaN and an inf vertex, and an isolated vertex.  -> (verts, faces)"""
    rng = np.random.default_rng(21)
    n = 5
    idx = lambda i, j: i * n + j
    v = [[i + 0.2 * rng.random(), j + 0.2 * rng.random(), 0.3 * rng.random()] for i in range(n) for j in range(n)]
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [[a, b, c], [a, d, c] if (i, j) == (2, 1) else [a, c, d]]
    v += [[1.5, 1.5, 1.0], [9.0, 9.0, 9.0]]  # the fin's tip, an isolated vertex
    tip = n * n
    f.append([idx(1, 1), idx(2, 2), tip])  # a third face on the diagonal of quad (1, 1)
    V = len(v)
    f += [[3, 3, 4], [0, 1, -1], [1, 2, V], [2, 3, 2 ** 31 - 1]]
    v = np.asarray(v, dtype=F32)
    v[idx(3, 3), 1] = np.nan
    v[idx(0, 2), 0] = np.inf
    f = np.asarray(f, dtype=np.int64).astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f
