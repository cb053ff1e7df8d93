"""numpy restatement of the mesh-component calls (include/nerf_hip.h, "Connected components of an indexed triangle mesh"): a plain
union-find for the labels, and the counts, boxes, selection and compaction defined on top of them.  The device results are held to
these bit for bit (tests/test_gpu_mesh_components.py); tests/test_mesh_components_cpu.py holds this file to a brute-force flood fill."""
import numpy as np


def valid_faces(faces, V):
    """[F] bool: every index of the face lies in [0, V)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def labels(faces, V):
    """[V] int64: the smallest vertex index of each vertex's component (union-find; the lower root always wins)."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    for a, b, c in f[valid_faces(f, V)].tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    return np.array([find(v) for v in range(V)], dtype=np.int64).reshape(V)


def components(faces, V, verts=None):
    """-> dict(vert_comp [V] int32, face_comp [F] int32, n_verts [C] int32, n_faces [C] int32, bbox_lo / bbox_hi [C, 3] fp32 or None, C)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lab = labels(f, V)
    roots = np.flatnonzero(lab == np.arange(V))  # ascending: the ids' order
    C = len(roots)
    rid = np.full(V, -1, np.int64)
    rid[roots] = np.arange(C)
    vert_comp = rid[lab].astype(np.int32).reshape(V)
    ok = valid_faces(f, V)
    face_comp = np.full(len(f), -1, np.int32)
    face_comp[ok] = vert_comp[f[ok, 0]]
    n_verts = np.bincount(vert_comp, minlength=C).astype(np.int32)
    n_faces = np.bincount(face_comp[ok], minlength=C).astype(np.int32)
    lo = hi = None
    if verts is not None:
        x = np.array(verts, dtype=np.float32).reshape(V, 3)
        x[x == 0] = 0.0  # -0 counts as +0
        lo = np.full((C, 3), np.inf, np.float32)
        hi = np.full((C, 3), -np.inf, np.float32)
        for d in range(3):
            fin = np.isfinite(x[:, d])  # a coordinate that is not finite is ignored
            np.minimum.at(lo[:, d], vert_comp[fin], x[fin, d])
            np.maximum.at(hi[:, d], vert_comp[fin], x[fin, d])
    return dict(vert_comp=vert_comp, face_comp=face_comp, n_verts=n_verts, n_faces=n_faces, bbox_lo=lo, bbox_hi=hi, C=C)


def select(n_faces, min_faces=1, keep_largest=None):
    """[C] bool: n_faces >= min_faces and, with keep_largest = k, among the k components with the most faces (ties: the lower id)."""
    n = np.asarray(n_faces, dtype=np.int64)
    keep = n >= min_faces
    if keep_largest is not None:
        order = sorted(range(len(n)), key=lambda c: (-n[c], c))
        top = np.zeros(len(n), bool)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def compact(verts, faces, vert_comp, face_comp, keep, normals=None, rgb=None):
    """-> (verts', faces' int32, normals' or None, rgb' or None): kept vertices and faces in their order, indices renumbered."""
    keep = np.asarray(keep, dtype=bool)
    vert_comp, face_comp = np.asarray(vert_comp), np.asarray(face_comp)
    kv = keep[vert_comp] if len(vert_comp) else np.zeros(0, bool)
    kf = np.zeros(len(face_comp), bool)
    kf[face_comp >= 0] = keep[face_comp[face_comp >= 0]]
    newidx = np.cumsum(kv) - 1
    f = np.asarray(faces).reshape(-1, 3)[kf]
    take = lambda a: None if a is None else np.asarray(a).reshape(-1, 3)[kv]
    return take(verts), newidx[f].astype(np.int32).reshape(-1, 3), take(normals), take(rgb)


def hook_rounds(faces, V, cap=64):
    """Rounds that the SYNCHRONOUS restatement of the device's labelling needs, the last one changing nothing (every face reads the
    labels as the round found them; the device, whose faces see each other's atomics, may need fewer or more).  -> (rounds, labels)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    L = np.arange(V)
    for rounds in range(1, cap + 1):
        r = L[f]  # roots: every round starts fully compressed
        m = r.min(axis=1, keepdims=True)
        new = L.copy()
        np.minimum.at(new, r.reshape(-1), np.broadcast_to(m, r.shape).reshape(-1))
        changed = not np.array_equal(new, L)
        L = new
        while True:  # compress
            nxt = L[L]
            if np.array_equal(nxt, L):
                break
            L = nxt
        if not changed:
            return rounds, L
    raise RuntimeError(f"no fixed point in {cap} rounds")
