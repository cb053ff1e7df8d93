"""A numpy restatement of rules TA and TX of include/nerf_hip.h (texture atlases of indexed meshes): the atlas's sizes, ownership and
integer weights, the texels' points and directions with fp32 operations in the header's order, the UV table, and the bilinear
lookup in fp64 in its fixed order.  No device and no library: the GPU tests compare the kernels with these arrays bit for bit, the
CPU tests hold the rule's two properties (no bleeding between faces; linear colours come back exactly) on them."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def dims(F, n):
    """-> (c, Sx, Sy, W, H)"""
    c, K = n + 5, (F + 1) // 2
    Sx = math.isqrt(K)
    if Sx * Sx < K:
        Sx += 1
    Sy = (K + Sx - 1) // Sx if Sx else 0
    return c, Sx, Sy, Sx * c, Sy * c


def lower_weights(i, j, n):
    """the integer weights (w0, u, v) * 2n of the cell-local texel (i, j) of a LOWER chart, and whether it is a support texel"""
    a, b = i - 1, j - 1
    if a >= 0 and b >= 0 and a + b <= n + 1:
        return (2 * n - 2 * a - 2 * b, 2 * a, 2 * b), True
    a, b = min(max(a, 0), n), min(max(b, 0), n)
    un, vn = (a - b + n, b - a + n) if a + b > n else (2 * a, 2 * b)
    return (2 * n - un - vn, un, vn), False


def owner(F, n):
    """-> (face [H, W] int64: the face that owns each texel, -1 where none does; wts [H, W, 3] int64: its weights * 2n in the face's own
    (reflected) frame; support [H, W] bool)"""
    c, Sx, Sy, W, H = dims(F, n)
    face = np.full((H, W), -1, np.int64)
    wts = np.zeros((H, W, 3), np.int64)
    support = np.zeros((H, W), bool)
    table = {(i, j): lower_weights(i, j, n) for i in range(c) for j in range(c) if i + j <= c - 1}
    for y in range(H):
        for x in range(W):
            cx, cy = x // c, y // c
            i, j = x - cx * c, y - cy * c
            upper = int(i + j >= c)
            if upper:
                i, j = c - 1 - i, c - 1 - j
            f = 2 * (cy * Sx + cx) + upper
            if f < F:
                face[y, x] = f
                wts[y, x], support[y, x] = table[(i, j)]
    return face, wts, support


def uv_table(F, n):
    """-> [F, 3, 2] fp32: per face and corner (x / W, y / H), y down; the numerators are the half-integer texel coordinates as fp32"""
    c, Sx, Sy, W, H = dims(F, n)
    out = np.zeros((F, 3, 2), F32)
    local = [(1.5, 1.5), (1.5 + n, 1.5), (1.5, 1.5 + n)]
    for f in range(F):
        k = f >> 1
        cx, cy = k % Sx, k // Sx
        for q, (x, y) in enumerate(local):
            if f & 1:
                x, y = c - x, c - y
            out[f, q] = F32(cx * c + x) / F32(W), F32(cy * c + y) / F32(H)
    return out


def texels(verts, normals, faces, n, row0=0, rows=None):
    """rule TA -> (points [rows, W, 3], dirs [rows, W, 3] fp32, mask [rows, W] uint8) of the atlas rows [row0, row0 + rows)"""
    verts, normals = np.asarray(verts, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    c, Sx, Sy, W, H = dims(F, n)
    rows = H - row0 if rows is None else rows
    face, wts, _ = owner(F, n)
    P, D, M = np.zeros((rows, W, 3), F32), np.zeros((rows, W, 3), F32), np.zeros((rows, W), np.uint8)
    den = F32(2 * n)
    with np.errstate(all="ignore"):
        for y in range(row0, row0 + rows):
            for x in range(W):
                f = face[y, x]
                if f < 0:
                    continue
                idx = faces[f]
                if (idx < 0).any() or (idx >= V).any():
                    continue
                M[y - row0, x] = 1
                w = wts[y, x]
                if (w == 0).sum() == 2:  # on a vertex: its position and normal as they are
                    one = idx[int(np.argmax(w != 0))]
                    P[y - row0, x] = verts[one]
                    if np.isfinite(normals[one]).all():
                        D[y - row0, x] = -normals[one]
                    continue
                w0, u, v = F32(w[0]) / den, F32(w[1]) / den, F32(w[2]) / den
                A, B, C = verts[idx]
                nA, nB, nC = normals[idx]
                P[y - row0, x] = w0 * A + (u * B + v * C)
                nb = w0 * nA + (u * nB + v * nC)
                L = np.sqrt((nb[0] * nb[0] + nb[1] * nb[1]) + nb[2] * nb[2])
                if np.isfinite(L) and L > 0:
                    D[y - row0, x] = -(nb / L)
    return P, D, M


def sample(image, F, n, face, uv, background=(0.0, 0.0, 0.0), touched=None):
    """rule TX -> (rgb [N, 3] fp32, valid [N] uint8).  touched: a list that receives, per valid lookup, the (y, x, weight) of the texels
    read.  image may be fp64 (the CPU tests' exact colours): the arithmetic is fp64 either way and the result is returned unrounded
    then."""
    image = np.asarray(image)
    c, Sx, Sy, W, H = dims(F, n)
    face, uv = np.asarray(face, np.int64).reshape(-1), np.asarray(uv, F64).reshape(-1, 2)
    N = len(face)
    rgb = np.zeros((N, 3), image.dtype)
    valid = np.zeros(N, np.uint8)
    for q in range(N):
        f, (u, v) = int(face[q]), uv[q]
        if f < 0 or f >= F or not np.isfinite(u) or not np.isfinite(v):
            rgb[q] = np.asarray(background, F32)
            continue
        valid[q] = 1
        u = min(max(u, 0.0), 1.0)
        v = min(max(v, 0.0), F64(1.0) - u)
        tx, ty = F64(1.0) + u * F64(n), F64(1.0) + v * F64(n)
        fi, fj = min(np.floor(tx), F64(c - 2)), min(np.floor(ty), F64(c - 2))
        fx, fy = tx - fi, ty - fj
        k, upper = f >> 1, f & 1
        bx, by = (k % Sx) * c, (k // Sx) * c
        acc = np.zeros(3, F64)
        for dj in range(2):
            for di in range(2):
                w = (fx if di else F64(1.0) - fx) * (fy if dj else F64(1.0) - fy)
                if w == 0.0:
                    continue
                i, j = int(fi) + di, int(fj) + dj
                X, Y = bx + (c - 1 - i if upper else i), by + (c - 1 - j if upper else j)
                if touched is not None:
                    touched.append((q, Y, X, w))
                acc = acc + w * image[Y, X].astype(F64)
        rgb[q] = acc.astype(image.dtype)
    return rgb, valid


def random_mesh(F, V, seed):
    """a random indexed mesh with unit normals, then the hard cases: a face with an index outside [0, V), a vertex with NaN and inf
    coordinates, a vertex with a NaN normal, a zero normal and two opposite normals on one face (a blend of length 0)"""
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1.0, 1.0, (V, 3)).astype(F32)
    g = rng.standard_normal((V, 3)).astype(F32)
    normals = (g / np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])[:, None]).astype(F32)
    faces = rng.integers(0, V, (F, 3)).astype(np.int32)
    if F >= 5:
        faces[1] = (0, V, 1)
        faces[2, 0] = -1
        verts[faces[3, 0]] = (np.nan, np.inf, 0.25)
        normals[faces[4, 1]] = 0.0
        normals[faces[4, 2]] = (np.nan, 0.0, 1.0)
        faces[0] = (V - 1, V - 2, V - 2)
        normals[V - 1] = (0.0, 0.6, 0.8)
        normals[V - 2] = (0.0, -0.6, -0.8)
    return verts, normals, faces


def barycentrics(count, seed):
    """(u, v) [.., 2] fp64 inside the triangle: the corners, the edge midpoints, points on the edges, then random interior points"""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.25, 0.75), (0.3, 0.0), (0.0, 0.7)]
    r = rng.random((count, 2))
    flip = r.sum(1) > 1
    r[flip] = 1.0 - r[flip]
    return np.concatenate((np.array(fixed, F64), r))
