"""The mesh semantics of nerf_hip_mesh_count / nerf_hip_mesh_emit (include/nerf_hip.h) restated in vectorised numpy
fp32, with the triangle table read from nerf-tiny_amd/csrc/mc_tables.h.  Used by tests/test_mesh_cpu.py and tests/test_gpu_mesh.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_H = os.path.join(ROOT, "nerf-tiny_amd", "csrc", "mc_tables.h")

# corner c -> (dx, dy, dz) offset from the cell's lowest lattice point (i, j, k); x is the slowest grid axis, z the fastest
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], dtype=np.int64)
# edge e -> (corner, corner), as the header states them
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def _edge_owner_axis():
    own, axis = np.zeros((12, 3), np.int64), np.zeros(12, np.int64)
    for e, (a, b) in enumerate(EDGES):
        d = CORNERS[b] - CORNERS[a]
        assert np.abs(d).sum() == 1
        axis[e] = int(np.nonzero(d)[0][0])
        own[e] = np.minimum(CORNERS[a], CORNERS[b])  # the lower endpoint owns the edge's vertex
    return own, axis


EDGE_OWNER, EDGE_AXIS = _edge_owner_axis()


def load_table(path=TABLE_H):
    """mc_tri_table[256][16] from the header: the body of the one brace-initialised array, -1 padded."""
    src = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(path).read(), flags=re.S)
    m = re.search(r"mc_tri_table\s*\[\s*256\s*\]\s*\[\s*16\s*\]\s*=\s*\{(.*?)\};", src, flags=re.S)
    assert m, "mc_tri_table[256][16] not found"
    vals = [int(v) for v in re.findall(r"-?\d+", m.group(1))]
    assert len(vals) == 256 * 16, len(vals)
    return np.array(vals, dtype=np.int64).reshape(256, 16)


def cube_index(inside_corners):
    """Bit c of a cell's table row is set when corner c is OUTSIDE (sigma <= level or NaN), the table's "below the isovalue"."""
    idx = 0
    for c in range(8):
        if not inside_corners[c]:
            idx |= 1 << c
    return idx


def _gradient(s, step):
    """Central differences (s[+1] - s[-1]) / (2 step_a) inside, one-sided / step_a at the grid's faces (every dimension >= 2)."""
    g = np.empty((3,) + s.shape, np.float32)
    for a in range(3):
        sa = np.moveaxis(s, a, 0)
        ga = np.moveaxis(g[a], a, 0)
        ga[1:-1] = (sa[2:] - sa[:-2]) / (np.float32(2) * step[a])
        ga[0] = (sa[1] - sa[0]) / step[a]
        ga[-1] = (sa[-1] - sa[-2]) / step[a]
    return g


def marching_cubes(sigma, level, lo=(0, 0, 0), step=(1, 1, 1), table=None):
    """-> verts [V, 3] fp32, faces [F, 3] int32, normals [V, 3] fp32, with the vertex, face and rounding rules of the C ABI."""
    s = np.ascontiguousarray(sigma, dtype=np.float32)
    nx, ny, nz = s.shape
    level = np.float32(level)
    lo = np.asarray(lo, np.float32).reshape(3)
    step = np.asarray(step, np.float32).reshape(3)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    if min(nx, ny, nz) < 2:
        return empty
    table = load_table() if table is None else table
    N = nx * ny * nz
    strides = (ny * nz, nz, 1)
    with np.errstate(all="ignore"):
        inside = s > level  # NaN is outside
        own = np.zeros((nx, ny, nz, 3), bool)
        own[:-1, :, :, 0] = inside[:-1] != inside[1:]
        own[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
        own[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
        own = own.reshape(N, 3)
        p, ax = np.nonzero(own)  # row-major: by lower endpoint, then axis
        V = p.size
        vid = np.full((N, 3), -1, np.int32)
        vid[p, ax] = np.arange(V, dtype=np.int32)
        flat = s.reshape(-1)
        q = p + np.asarray(strides, np.int64)[ax]
        sa, sb = flat[p], flat[q]
        t = (level - sa) / (sb - sa)
        t = np.where(np.isfinite(t), t, np.float32(0.5)).astype(np.float32)
        ijk = np.stack(np.unravel_index(p, (nx, ny, nz)), axis=1)
        pa = lo + ijk.astype(np.float32) * step  # one fp32 product, one fp32 sum per coordinate
        verts = pa.copy()
        rows = np.arange(V)
        pb_ax = lo[ax] + (ijk[rows, ax] + 1).astype(np.float32) * step[ax]
        verts[rows, ax] = pa[rows, ax] + t * (pb_ax - pa[rows, ax])
        g = _gradient(s, step).reshape(3, N)
        ga, gb = g[:, p].T, g[:, q].T
        gv = ga + t[:, None] * (gb - ga)
        norm = np.sqrt(gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1] + gv[:, 2] * gv[:, 2])
        ok = np.isfinite(norm) & (norm > 0)
        normals = np.where(ok[:, None], -gv / np.where(ok, norm, np.float32(1))[:, None], np.float32(0)).astype(np.float32)

        cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
        for c, (dx, dy, dz) in enumerate(CORNERS):
            cube |= (~inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]).astype(np.int64) << c
    ntri = (table >= 0).sum(axis=1) // 3
    cube = cube.reshape(-1)
    nt = ntri[cube]
    cells = np.repeat(np.arange(cube.size), nt)  # C order over cells, then table order within the entry
    within = np.arange(cells.size) - np.repeat(np.cumsum(nt) - nt, nt)
    edges = table[cube[cells][:, None], 3 * within[:, None] + np.arange(3)[None, :]]  # [F, 3] edge ids
    ci = np.stack(np.unravel_index(cells, (nx - 1, ny - 1, nz - 1)), axis=1)
    o = ci[:, None, :] + EDGE_OWNER[edges]
    lin = (o[..., 0] * ny + o[..., 1]) * nz + o[..., 2]
    faces = vid[lin, EDGE_AXIS[edges]]
    assert (faces >= 0).all(), "a face uses an edge without a vertex: the table and the vertex rule disagree"
    return verts.astype(np.float32), faces.astype(np.int32), normals


def mesh_stats(verts, faces):
    """(directed edges each exactly once, Euler characteristic V - E + F over the used vertices, signed volume, area) in float64."""
    f = np.asarray(faces, np.int64)
    v = np.asarray(verts, np.float64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * (len(v) + 1) + d[:, 1]
    uniq, cnt = np.unique(key, return_counts=True)
    rev = d[:, 1] * (len(v) + 1) + d[:, 0]
    closed = bool((cnt == 1).all() and np.isin(rev, uniq).all())
    E = len(uniq) // 2
    Vu = len(np.unique(f))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    area = float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)
    return closed, Vu - E + len(f), vol, area
