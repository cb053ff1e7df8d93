"""CPU: the numpy restatement of the ray-casting rules (tests/raycast_reference.py) against its plain-loop reading of
include/nerf_hip.h; a unit cube with exact answers; the grid's sizing rule (mesh.raycast_grid) against the reference; the header,
the binding and the built library; and a scalar model of the interval walk of csrc/mesh_raycast.hip against brute force over
several grids -- the proof at the top of that file, checked."""
import ctypes
import os
import re

import numpy as np
import pytest

import raycast_reference as R
import simplify_meshes as M
from conftest import ROOT

F32 = np.float32
NEW_CALLS = ("nerf_hip_mesh_raycast_ws_bytes", "nerf_hip_mesh_raycast_grid_count", "nerf_hip_mesh_raycast_grid_fill", "nerf_hip_mesh_raycast",
             "nerf_hip_mesh_face_rays", "nerf_hip_mesh_select_faces_ws_bytes", "nerf_hip_mesh_select_faces_count",
             "nerf_hip_mesh_select_faces_emit")


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) and x.dtype == y.dtype
               for x, y in zip(a, b))


def _small(name):
    """a piece of a test mesh small enough for the loops: the faces around one spot, with the bad entries of bad_input kept"""
    v, f = (M.blobs() if name == "blobs" else M.bad_input())[:2]
    return v, f[:400]


# ---- restatement == loops ----

@pytest.mark.parametrize("name", ["blobs", "bad_input"])
def test_cast_restatement_equals_the_loops(name):
    v, f = _small(name)
    o, d = R.lattice_rays(v[np.unique(f[((f >= 0) & (f < len(v))).all(1)])], step=2.5)
    o2, d2 = R.random_rays(v, 40, 3)
    o3, d3 = R.bad_rays()
    ok = R.face_part(v, f)
    o4 = v[f[ok][:40, 0]]  # rays that start on a vertex: several faces at t = 0.0 and -0.0, which tie
    d4 = np.tile(np.array([[1, 0, 0], [0, -1, 0]], F32), (20, 1))
    o, d = np.concatenate((o, o2, o4, o3)), np.concatenate((d, d2, d4, d3))
    first = R.cast(v, f, o, d)
    assert (first[0] == 0).sum() >= 20
    assert (first[2] >= 0).sum() > 10 and _same(first, R.cast_loops(v, f, o, d))
    assert (first[2][-len(o3):][[1, 2, 3, 4, 5, 6]] == -1).all()
    skip = first[2].copy()
    for kw in (dict(tmin=3.0, tmax=9.5), dict(skip=skip), dict(tmin=-np.inf, tmax=np.inf), dict(tmin=2.0, tmax=1.0)):
        a = R.cast(v, f, o, d, **kw)
        assert _same(a, R.cast_loops(v, f, o, d, **kw)), kw
    assert not _same(first, R.cast(v, f, o, d, skip=skip)) and (R.cast(v, f, o, d, tmin=2.0, tmax=1.0)[2] == -1).all()


def test_grid_rays_and_selection_restatements_equal_the_loops():
    v, f = M.bad_input()[:2]
    f = f[:600]
    for lo, cell, dims in (((0, 0, 0), 1.0, (16, 16, 16)), ((2.5, 1.0, 3.0), 0.75, (9, 4, 30)), ((-50, -50, -50), 100.0, (1, 1, 1))):
        assert R.grid_counts(v, f, lo, cell, dims) == R.grid_counts_loops(v, f, lo, cell, dims)
    n = R.grid_counts(v, f, (0, 0, 0), 1.0, (16, 16, 16))
    assert 0 < n[2] < n[0] < len(f) and n[1] > n[0]
    pose = np.array([1, 0, 0, 8, 0, 0, 1, 0, 8, 0, 0, 0, 1, -20, 0, 2, 6], F32)
    Kinv = np.array([[0.05, 0, 0], [0, 0.05, 0], [-0.8, -0.8, 1]], F32)
    Q, cam = R.camera_q(pose, Kinv)
    a, b = R.face_rays(v, f, cam, Q, 32, 32), R.face_rays_loops(v, f, cam, Q, 32, 32)
    assert _same(a, b) and 0 < a[2].sum() < len(f)
    rng = np.random.default_rng(1)
    f = M.bad_input()[1]
    keep = (rng.random(len(f)) < 0.3) | ~((f >= 0) & (f < len(v))).all(1)
    nrm, rgb = rng.random((len(v), 3), dtype=F32), rng.random((len(v), 3), dtype=F32)
    a, b = R.select_faces(v, f, keep, nrm, rgb), R.select_faces_loops(v, f, keep, nrm, rgb)
    assert _same(a, b) and 0 < len(a[1]) < keep.sum()  # (kept faces with an index out of range go)


# ---- a unit cube: exact answers ----

def test_unit_cube_hits_are_exact():
    v, f = R.unit_cube()
    o = np.array([[-1, 0.25, 0.5], [2, 0.25, 0.5], [0.25, 0.5, -3], [0.5, 0.5, 0.5], [-1, -1, -1], [-1, 0.5, 0.5], [-1, 2, 0.5]], F32)
    d = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 2], [0, 1, 0], [1, 1, 1], [4, 0, 0], [1, 0, 0]], F32)
    t, uv, face, side = R.cast(v, f, o, d)
    assert t.tolist() == [1.0, 1.0, 1.5, 0.5, 1.0, 0.25, np.inf] and side.tolist() == [1, 1, 1, -1, 1, 1, 0]
    assert face.tolist() == [0, 3, 8, 6, 0, 0, -1]  # (the cube's corner and the faces' diagonals: the lowest face index)
    assert uv.tolist() == [[0.25, 0.25], [0.25, 0.25], [0.25, 0.25], [0.0, 0.5], [0.0, 0.0], [0.0, 0.5], [0.0, 0.0]]
    assert _same((t, uv, face, side), R.cast_loops(v, f, o, d))
    # the second hit of each ray: the far wall from inside
    t2 = R.cast(v, f, o, d, skip=face)[0]
    assert t2[0] == 2.0 and t2[5] == 0.25 and R.cast(v, f, o, d, tmin=1.25)[0][0] == 2.0  # (ray 5 runs along two faces' shared diagonal)
    assert R.cast(v, f, o, d, tmin=1.0, tmax=1.0)[2].tolist() == [0, 3, -1, -1, 0, -1, -1]  # the window's ends count


# ---- the sizing rule ----

@pytest.mark.parametrize("name", ["blobs", "random", "nothing_finite", "empty"])
def test_raycast_grid_rule(pkg, name):
    if name == "nothing_finite":
        v, f = np.full((5, 3), np.nan, F32), np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    elif name == "empty":
        v, f = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    else:
        v, f = (M.blobs() if name == "blobs" else M.random_mesh())[:2]
    asked = []

    def count(lo, cell, dims):
        asked.append((float(cell), tuple(dims)))
        return R.grid_counts(v, f, lo, cell, dims)[1]

    lo, cell, dims = pkg.mesh.raycast_grid(np.array(v), np.array(f), count=count)  # (copies: the fixtures are read-only)
    want = R.raycast_grid(v, f)
    assert np.array_equal(lo, want[0]) and lo.dtype == F32 and cell == want[1] and tuple(dims) == tuple(want[2])
    if name in ("blobs", "random"):
        n = R.grid_counts(v, f, lo, cell, dims)
        first = R.grid_counts(v, f, lo, asked[0][0], asked[0][1])
        print(f"{name}: F {len(f)}, first cell {asked[0][0]} dims {asked[0][1]} E/F {first[1] / len(f):.2f} -> cell {cell} dims {dims} E/F {n[1] / len(f):.2f}")
        assert n[2] == 0 and n[0] == len(f) and n[1] <= 4 * len(f) + 64 and len(asked) >= 1
        assert np.prod(asked[0][1]) <= 2 * len(f) + 8
    else:
        assert tuple(dims) == (1, 1, 1) and cell == 1 and not asked
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.raycast_grid(np.array(v), np.array(f))


def test_cpu_tensors_raise(pkg):
    import torch

    m = pkg.mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), None, None)
    for call in (lambda: pkg.mesh.build_raycast(m), lambda: pkg.mesh.visibility(m, torch.zeros(1, 17), torch.eye(3), 4, 4),
                 lambda: pkg.mesh.filter_faces(m, torch.ones(1)), lambda: pkg.mesh.raycast(None, torch.zeros(2, 3), torch.zeros(2, 3))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_camera_q_inverts_the_ray_rule(pkg):
    pose = np.array([0.36, 0.48, -0.8, 3, 0, -0.8, 0.6, 0, -2, 0, 0.48, 0.64, 0.6, 1, 0, 2, 6], F32)
    Kinv = np.array([[0.01, 0, 0], [0, 0.0125, 0], [-0.3, -0.4, 1]], F32)
    Q, cam = pkg.mesh.camera_q(pose, Kinv)
    Qr, camr = R.camera_q(pose, Kinv)
    assert np.array_equal(Q, Qr) and np.array_equal(cam, camr) and cam.tolist() == [3, -2, 1]
    x, y = 17.0, 40.0
    K = Kinv.reshape(-1).astype(np.float64)  # (the rule in exact arithmetic on the fp32 entries: fp64 here)
    p = np.array([(x * K[j] + y * K[3 + j]) + K[6 + j] for j in range(3)])
    m = Q @ (pose[:15].reshape(3, 5)[:, :3].astype(np.float64) @ p)
    assert abs(m[0] / m[2] - x) < 1e-9 and abs(m[1] / m[2] - y) < 1e-9 and m[2] > 0


# ---- the header, the binding, the library ----

def test_header_declares_the_calls_with_abi_7(pkg):
    src = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define NERF_HIP_ABI_VERSION 7\b", src) and pkg._abi.NERF_HIP_ABI_VERSION == 7
    assert "ABI 7 additions.  Rays against a mesh" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_CALLS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in pkg._abi.EXPORTS, name
    for helper in ("raycast_grid", "build_raycast", "raycast", "camera_rays", "render_depth", "visibility", "filter_faces"):
        assert callable(getattr(pkg.mesh, helper)), helper


def test_library_exports_the_calls(pkg):
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    for name in NEW_CALLS:
        assert hasattr(lib, name), name
    # the size calls run on the host: 8 bytes per cell, 4 per entry and per face, in whole 256-byte units
    small, big = pkg._abi.mesh_raycast_ws_bytes(100, 1000, (4, 4, 4)), pkg._abi.mesh_raycast_ws_bytes(100, 5000, (4, 4, 4))
    assert small % 256 == 0 and 16000 <= big - small <= 16256 and small >= 64 * 8 + 1000 * 4 + 100 * 4
    assert pkg._abi.mesh_select_faces_ws_bytes(1000, 10) >= 8000
    for fn, args in ((pkg._abi.mesh_raycast_ws_bytes, (-1, 0, (1, 1, 1))), (pkg._abi.mesh_raycast_ws_bytes, (1, 2 ** 31, (1, 1, 1))),
                     (pkg._abi.mesh_raycast_ws_bytes, (1, 1, (0, 1, 1))), (pkg._abi.mesh_raycast_ws_bytes, (1, 1, (2048, 2048, 512))),
                     (pkg._abi.mesh_select_faces_ws_bytes, (-1, 0)), (pkg._abi.mesh_select_faces_ws_bytes, (0, 2 ** 31))):
        with pytest.raises(pkg._abi.NerfHipError):
            fn(*args)


# ---- the interval walk equals brute force, for every grid ----

def _walk_rays(v, grid):
    o, d = R.lattice_rays(v, step=5.5)
    o2, d2 = R.random_rays(v, 24, 7)
    lo, hi = R._box(v)
    o3, d3 = R.random_rays(v, 10, 8, inside=(lo + hi) / 2)
    o4, d4 = R.plane_rays(grid, n=3)
    o5, d5 = R.bad_rays()
    far = (o2[:8].astype(np.float64) + d2[:8] * -2000.0).astype(F32)  # the same lines from far outside the grid
    return (np.concatenate((o, o2, o3, o4[::7], o5, far, o2[:8])),
            np.concatenate((d, d2, d3, d4[::7], d5, d2[:8], d2[:8] * F32(1e-3))))


@pytest.mark.parametrize("name", ["blobs", "bad_input"])
def test_walk_model_equals_brute_force_over_several_grids(name):
    if name == "blobs":
        v, f = M.blobs()[:2]
    else:  # a piece of it: vertices that are not finite or far away, indices out of range
        v, f = M.bad_input()[:2]
        f = f[np.r_[0:900, np.flatnonzero(~((f >= 0) & (f < len(v))).all(1))[:40]]]
    default = R.raycast_grid(v, f)
    ok = ((f >= 0) & (f < len(v))).all(1)
    v_used = v[np.unique(f[ok])]
    lo, hi = R._box(v_used)
    regular = (lo - F32(0.01), F32(1.4), (17, 17, 17))
    mid = np.median(v_used[np.isfinite(v_used).all(1), 0])  # a grid that starts here leaves about half the faces OUTSIDE
    grids = {"default": default, "regular": regular, "one cell": (lo, 1.0, (1, 1, 1)), "flat": (lo - F32(0.5), 5.0, (37, 1, 5)),
             "tiny cells": (lo + F32(4.0), 0.2, (64, 64, 64)), "shifted": (np.array([mid, lo[1] - 0.01, lo[2] - 0.01], F32), regular[1], regular[2])}
    for gname, grid in grids.items():
        o, d = _walk_rays(v_used, grid if gname != "one cell" else regular)
        want = R.cast(v, f, o, d)
        stats = {}
        got = R.walk_model(v, f, grid, o, d, stats=stats)
        n = R.grid_counts(v, f, *grid)
        print(f"{name} / {gname}: {len(o)} rays, {int((want[2] >= 0).sum())} hit, grid E {n[1]} OUTSIDE {n[2]} of {n[0]}, "
              f"{stats.get('tests', 0) / len(o):.1f} faces per ray of {len(f)}")
        assert _same(got, want), gname
        assert (want[2] >= 0).sum() > 15
        if gname == "regular":
            assert stats["tests"] < 0.05 * len(o) * len(f) and n[2] <= (0 if name == "blobs" else 60)  # the grid does its work
        if gname == "one cell":
            assert n[2] == n[0]  # brute force through the OUTSIDE list
        if gname == "shifted":
            assert 0.2 * n[0] < n[2] < 0.9 * n[0]  # about half the faces are OUTSIDE
        if gname in ("regular", "shifted"):
            sub = slice(None, None, 2)
            for kw in (dict(tmin=5.0, tmax=14.0), dict(skip=want[2][sub].copy()), dict(tmin=-np.inf)):
                assert _same(R.walk_model(v, f, grid, o[sub], d[sub], **kw), R.cast(v, f, o[sub], d[sub], **kw)), (gname, kw)
