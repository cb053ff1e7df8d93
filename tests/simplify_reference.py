"""numpy restatement of the vertex-clustering simplification (include/nerf_hip.h): simplify() vectorised,
simplify_loops() a plain-loop reading of the same definition (tests/test_mesh_simplify_cpu.py holds one against the other), and the
default lattice of mesh.simplify."""
import numpy as np

F32 = np.float32
POS_ONE = float(2 ** 20)
NRM_ONE = float(2 ** 28)
MAX_DIM = 2048


def lattice(lo, cell, dims):
    lo = np.asarray(lo, dtype=F32).reshape(3)
    cell = np.broadcast_to(np.asarray(cell, dtype=F32), (3,)).copy()
    dims = np.asarray(dims, dtype=np.int64).reshape(3)
    assert np.isfinite(lo).all() and (cell > 0).all() and np.isfinite(cell).all()
    assert (dims >= 1).all() and (dims <= MAX_DIM).all() and int(np.prod(dims)) < 2 ** 31
    return lo, cell, dims


def default_lattice(verts, cell, lo=None):
    """mesh.simplify_lattice: lo = the minimum over the finite vertices (unless given), dims = clamp(floor(fp32(fp32(hi - lo) / cell)) +
    1, 1, 2048) with hi their maximum."""
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    cell = np.broadcast_to(np.asarray(cell, dtype=F32), (3,)).copy()
    ok = np.isfinite(v).all(1)
    if not ok.any():
        return (np.zeros(3, F32) if lo is None else np.asarray(lo, F32).reshape(3)), cell, np.ones(3, np.int64)
    lo = v[ok].min(0) if lo is None else np.asarray(lo, F32).reshape(3)
    hi = v[ok].max(0)
    with np.errstate(all="ignore"):
        u = ((hi - lo).astype(F32) / cell).astype(F32)
        dims = np.clip(np.floor(u.astype(np.float64)) + 1, 1, MAX_DIM)
    return lo, cell, np.where(np.isnan(dims), 1, dims).astype(np.int64)


def vertex_cells(verts, lo, cell, dims):
    """-> (cell index [V] int64, -1 for a vertex in no cluster; uc [V, 3] fp32 clamped lattice coordinates)"""
    lo, cell, dims = lattice(lo, cell, dims)
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    d32 = dims.astype(F32)
    with np.errstate(all="ignore"):
        u = ((v - lo).astype(F32) / cell).astype(F32)
        u = np.where(np.isnan(u), F32(0), u)
        uc = np.minimum(np.maximum(u, F32(0)), d32).astype(F32)
        i = np.minimum(np.floor(uc), d32 - 1).astype(np.int64)
    lin = (i[:, 0] * dims[1] + i[:, 1]) * dims[2] + i[:, 2]
    ok = np.isfinite(v).all(1)
    return np.where(ok, lin, -1), uc


def _rotate_min_first(t):
    k = np.argmin(t, axis=1)
    idx = (k[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(t, idx, axis=1)


def simplify(verts, faces, normals, lo, cell, dims):
    """-> dict(verts [V', 3] fp32, faces [F', 3] int32, normals [V', 3] fp32 or None, clusters, degenerate_faces, duplicate_faces,
    kept [F'] input indices of the kept faces, cells [V'] cell index of every output vertex, unreferenced (occupied clusters no kept
    face uses), opposite_pairs (kept faces whose reversed triple is kept too, counted once per pair))"""
    lo, cell, dims = lattice(lo, cell, dims)
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    lin, uc = vertex_cells(v, lo, cell, dims)
    member = lin >= 0
    occupied = np.unique(lin[member])
    cid = np.searchsorted(occupied, np.where(member, lin, 0))  # cluster id of a member
    C = len(occupied)
    # sums
    n = np.zeros(C, np.int64)
    S = np.zeros((C, 3), np.int64)
    np.add.at(n, cid[member], 1)
    np.add.at(S, cid[member], np.rint(uc[member].astype(np.float64) * POS_ONE).astype(np.int64))
    T = None
    if normals is not None:
        nr = np.asarray(normals, dtype=F32).reshape(-1, 3)
        good = member & np.isfinite(nr).all(1)
        T = np.zeros((C, 3), np.int64)
        with np.errstate(all="ignore"):
            t = np.rint(np.clip(nr[good], F32(-2), F32(2)).astype(np.float64) * NRM_ONE).astype(np.int64)
        np.add.at(T, cid[good], t)
    # faces
    inr = ((f >= 0) & (f < V)).all(1)
    fc = np.where(inr[:, None], lin[np.where(inr[:, None], f, 0)], -1) if V > 0 else np.full_like(f, -1)
    part = inr & (fc >= 0).all(1)
    degen = part & ((fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2]))
    cand = np.flatnonzero(part & ~degen)
    canon = _rotate_min_first(fc[cand])
    if len(cand):
        _, first = np.unique(canon, axis=0, return_index=True)
        kept = cand[np.sort(first)]
    else:
        kept = cand
    used = np.unique(fc[kept])  # cell indices of the referenced clusters, ascending
    out_faces = np.searchsorted(used, fc[kept]).astype(np.int32).reshape(-1, 3)
    uid = np.searchsorted(occupied, used)
    with np.errstate(all="ignore"):
        mean = S[uid].astype(np.float64) / (n[uid].astype(np.float64) * POS_ONE)[:, None]
        out_verts = (lo.astype(np.float64) + cell.astype(np.float64) * mean).astype(F32).reshape(-1, 3)
        out_normals = None
        if T is not None:
            t = T[uid].astype(np.float64)
            length = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])[:, None]
            out_normals = np.where(length > 0, t / np.where(length > 0, length, 1.0), 0.0).astype(F32).reshape(-1, 3)
    kc = _rotate_min_first(fc[kept]) if len(kept) else np.zeros((0, 3), np.int64)
    have = {tuple(r) for r in kc.tolist()}
    opposite = sum(1 for a, b, c in have if (a, c, b) in have) // 2
    return dict(verts=out_verts, faces=out_faces, normals=out_normals, clusters=C, degenerate_faces=int(degen.sum()),
                duplicate_faces=int(len(cand) - len(kept)), kept=kept, cells=used, unreferenced=int(C - len(used)), opposite_pairs=opposite)


def simplify_loops(verts, faces, normals, lo, cell, dims):
    """The definition read literally, one vertex and one face at a time -> (verts, faces, normals or None, clusters, degenerate_faces,
    duplicate_faces)."""
    lo, cell, dims = lattice(lo, cell, dims)
    v = np.asarray(verts, dtype=F32).reshape(-1, 3)
    V = len(v)
    cell_of = []
    n, S, T = {}, {}, {}
    with np.errstate(all="ignore"):
        for i in range(V):
            if not all(np.isfinite(v[i])):
                cell_of.append(-1)
                continue
            lin, s = 0, []
            for d in range(3):
                u = F32(F32(v[i, d] - lo[d]) / cell[d])
                uc = min(max(u, F32(0)), F32(dims[d]))
                lin = lin * int(dims[d]) + int(min(np.floor(uc), F32(dims[d] - 1)))
                s.append(int(np.rint(np.float64(uc) * POS_ONE)))
            cell_of.append(lin)
            n[lin] = n.get(lin, 0) + 1
            S[lin] = [a + b for a, b in zip(S.get(lin, [0, 0, 0]), s)]
            if normals is not None:
                nr = np.asarray(normals[i], dtype=F32)
                if all(np.isfinite(nr)):
                    t = [int(np.rint(np.float64(min(max(x, F32(-2)), F32(2))) * NRM_ONE)) for x in nr]
                    T[lin] = [a + b for a, b in zip(T.get(lin, [0, 0, 0]), t)]
    seen, kept, n_deg, n_dup = set(), [], 0, 0
    for j, face in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if any(not 0 <= a < V for a in face):
            continue
        c = [cell_of[a] for a in face]
        if min(c) < 0:
            continue
        if len(set(c)) < 3:
            n_deg += 1
            continue
        k = c.index(min(c))
        key = (c[k], c[(k + 1) % 3], c[(k + 2) % 3])
        if key in seen:
            n_dup += 1
            continue
        seen.add(key)
        kept.append(c)
    used = sorted({c for tri in kept for c in tri})
    new = {c: i for i, c in enumerate(used)}
    out_faces = np.asarray([[new[c] for c in tri] for tri in kept], dtype=np.int32).reshape(-1, 3)
    out_verts = np.zeros((len(used), 3), F32)
    out_normals = np.zeros((len(used), 3), F32) if normals is not None else None
    for i, c in enumerate(used):
        for d in range(3):
            mean = np.float64(S[c][d]) / (np.float64(n[c]) * POS_ONE)
            out_verts[i, d] = F32(np.float64(lo[d]) + np.float64(cell[d]) * mean)
        if normals is not None:
            t = [np.float64(x) for x in T.get(c, [0, 0, 0])]
            length = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
            if length > 0:
                out_normals[i] = [F32(x / length) for x in t]
    return out_verts, out_faces, out_normals, len(n), n_deg, n_dup
