"""Input meshes of the simplification tests (CPU and GPU), each built once: the three-ball "blobs" mesh and the random 16^3 mesh of
tests/test_gpu_mesh_components.py (the same fields, through the marching-cubes restatement), a fan, and a mesh with bad entries."""
import functools

import numpy as np

BALLS = (((6.3, 6.1, 6.4), 4.2), ((16.5, 7.2, 15.8), 5.3), ((9.1, 17.4, 12.2), 3.1))
ISLAND = (20, 20, 3)
ANISO = dict(lo=(0.25, -1.0, 0.0), cell=(2.0, 3.5, 1.25))  # the anisotropic lattice of the random mesh


@functools.lru_cache(maxsize=None)
def blobs():
    """-> (verts, faces, normals): three balls of different sizes and a one-cell island on a 24^3 grid with unit steps, level 0"""
    import mc_reference as MC

    g = np.arange(24, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    s = np.full((24, 24, 24), -1.0)
    for (cx, cy, cz), r in BALLS:
        s = np.maximum(s, r - np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    s[ISLAND] = 0.75
    v, f, n = MC.marching_cubes(s.astype(np.float32), 0.0, (0, 0, 0), (1, 1, 1))
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


@functools.lru_cache(maxsize=None)
def random_mesh():
    """-> (verts, faces, normals): a random field on a 16^3 grid with unit steps at level 0.5"""
    import mc_reference as MC

    s = np.random.default_rng(16).random((16, 16, 16), dtype=np.float32)
    v, f, n = MC.marching_cubes(s, 0.5, (0, 0, 0), (1, 1, 1))
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n


def grid_lattice(n, k):
    """Cells of k steps of an n^3 unit-step grid from the origin (extract_mesh's rule): lo, cell, dims"""
    return (0.0, 0.0, 0.0), (np.float32(k),) * 3, (max(1, int(np.ceil((n - 1) / k))),) * 3


@functools.lru_cache(maxsize=None)
def fan():
    """300 vertices in three cells of a (3, 1, 1) unit lattice, 3000 faces that each take one vertex per cell, alternating between the
    two cyclic orders: more than one workgroup of faces sharing two keys.  -> (verts, faces, lo, cell, dims)"""
    rng = np.random.default_rng(5)
    cell_of = np.repeat(np.arange(3), 100)
    v = rng.random((300, 3), dtype=np.float32) * np.float32(0.9)
    v[:, 0] += cell_of.astype(np.float32)
    pick = rng.integers(0, 100, (3000, 3))
    f = pick + np.array([0, 100, 200])
    rot = rng.integers(0, 3, 3000)
    f = np.take_along_axis(f, (rot[:, None] + np.arange(3)) % 3, axis=1)  # any rotation: the same orientation
    f[1::2] = f[1::2, ::-1]  # every other face reversed
    f = f.astype(np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 1, 1)


@functools.lru_cache(maxsize=None)
def bad_input():
    """The random mesh with coordinates and normals that are not finite, vertices outside the lattice, and faces with indices -1, V
    and 2^31 - 1.  -> (verts, faces, normals, lo, cell, dims)"""
    v, f, n = (a.copy() for a in random_mesh())
    rng = np.random.default_rng(9)
    V, F = len(v), len(f)
    rows = rng.choice(V, 90, replace=False)
    v[rows[:20], rng.integers(0, 3, 20)] = np.nan
    v[rows[20:30], rng.integers(0, 3, 10)] = np.inf
    v[rows[30:40], rng.integers(0, 3, 10)] = -np.inf
    v[rows[40:60]] += np.float32(40.0)   # far outside, above
    v[rows[60:70]] -= np.float32(1e30)   # far outside, below
    n[rows[70:80], rng.integers(0, 3, 10)] = np.nan
    n[rows[80:90], rng.integers(0, 3, 10)] = np.inf
    n[rng.choice(V, 10, replace=False)] *= np.float32(100.0)  # clamped to [-2, 2]
    bad = rng.choice(F, 60, replace=False)
    f[bad, rng.integers(0, 3, 60)] = np.resize(np.array([-1, V, 2 ** 31 - 1], np.int64), 60).astype(np.int32)
    for a in (v, f, n):
        a.setflags(write=False)
    return v, f, n, (1.5, 1.0, 2.0), (np.float32(2.5),) * 3, (5, 5, 4)
