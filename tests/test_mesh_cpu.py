"""CPU: the marching-cubes table (csrc/mc_tables.h) is a valid table, the numpy restatement (tests/mc_reference.py) matches hand-worked
cases, write_ply round-trips, the mesh entry points refuse bad arguments before any device work, and the driver parses --mesh."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import mc_reference as R
from conftest import ROOT

MESH_SYMBOLS = ("nerf_hip_mesh_ws_bytes", "nerf_hip_mesh_count", "nerf_hip_mesh_emit")


def _tris(row):
    n = 0
    while n < 16 and row[n] >= 0:
        n += 1
    return n, [tuple(int(e) for e in row[t:t + 3]) for t in range(0, n - n % 3, 3)]


def _cube_faces(e):
    """The cube faces (axis, side) that contain edge e."""
    a, b = R.EDGES[e]
    ca, cb = R.CORNERS[a], R.CORNERS[b]
    return {(ax, int(ca[ax])) for ax in range(3) if ca[ax] == cb[ax]}


def _trilinear_grad(vals, x):
    g = np.zeros(3)
    for c in range(8):
        d = R.CORNERS[c]
        w = [x[k] if d[k] else 1.0 - x[k] for k in range(3)]
        sgn = [1.0 if d[k] else -1.0 for k in range(3)]
        g += vals[c] * np.array([sgn[0] * w[1] * w[2], w[0] * sgn[1] * w[2], w[0] * w[1] * sgn[2]])
    return g


def test_table_is_a_valid_marching_cubes_table():
    T = R.load_table()
    assert T.shape == (256, 16)
    for row_idx in range(256):
        row = T[row_idx]
        n, tris = _tris(row)
        # at most 5 triangles, then -1 padding
        assert n % 3 == 0 and n <= 15 and (row[n:] == -1).all(), row_idx
        inside = [not ((row_idx >> c) & 1) for c in range(8)]  # bit c set: corner c outside
        assert R.cube_index(inside) == row_idx
        # the edges used are exactly the edges whose ends differ
        want = {e for e, (a, b) in enumerate(R.EDGES) if inside[a] != inside[b]}
        assert {e for t in tris for e in t} == want, row_idx
        directed = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
        assert len(set(directed)) == len(directed), row_idx
        for a, b in directed:
            if (b, a) not in directed:
                # a boundary edge of the patch joins two cube edges of one common cube face
                assert _cube_faces(a) & _cube_faces(b), (row_idx, a, b)
        # (a shared edge appears once in each direction: no directed edge twice, and every undirected edge at most twice)
        und = {}
        for a, b in directed:
            und[frozenset((a, b))] = und.get(frozenset((a, b)), 0) + 1
        assert max(und.values(), default=0) <= 2, row_idx
        # orientation: with inside corners at 1 and outside at 0 (level 0.5, vertices at edge midpoints), the area-weighted
        # normals point down the trilinear interpolant's gradient
        vals = np.array([1.0 if i else 0.0 for i in inside])
        P = np.array([(R.CORNERS[a] + R.CORNERS[b]) / 2.0 for a, b in R.EDGES])
        tot = 0.0
        for t in tris:
            v0, v1, v2 = P[list(t)]
            tot += np.cross(v1 - v0, v2 - v0) @ _trilinear_grad(vals, (v0 + v1 + v2) / 3.0)
        if tris:
            assert tot < 0, (row_idx, tot)
    assert (T[0] == -1).all() and (T[255] == -1).all()


def test_reference_one_corner_inside():
    s = np.zeros((2, 2, 2), np.float32)
    s[0, 0, 0] = 3.0  # level 1: t = (1 - 3) / (0 - 3) = 2/3 along every edge out of the corner
    v, f, n = R.marching_cubes(s, 1.0, lo=(10, 20, 30), step=(2, 4, 8))
    t = np.float32(1 - 3) / np.float32(0 - 3)
    x = np.float32(10) + t * (np.float32(12) - np.float32(10))
    y = np.float32(20) + t * (np.float32(24) - np.float32(20))
    z = np.float32(30) + t * (np.float32(38) - np.float32(30))
    # vertices ordered by their lower endpoint (all at point 0), then x < y < z
    assert np.array_equal(v, np.float32([[x, 20, 30], [10, y, 30], [10, 20, z]]))
    assert f.shape == (1, 3) and sorted(f[0].tolist()) == [0, 1, 2]
    a, b, c = v[f[0]].astype(np.float64)
    nrm = np.cross(b - a, c - a)
    assert (nrm > 0).all()  # toward decreasing sigma: away from the dense corner
    assert (n > 0).all() and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)


def test_reference_plane():
    s = np.zeros((2, 2, 2), np.float32)
    s[0] = 1.0  # x = 0 inside, x = 1 outside: the plane x = 0.5, facing +x
    v, f, n = R.marching_cubes(s, 0.5)
    assert np.array_equal(v, np.float32([[0.5, 0, 0], [0.5, 0, 1], [0.5, 1, 0], [0.5, 1, 1]]))
    assert np.array_equal(n, np.float32([[1, 0, 0]] * 4))
    assert f.shape == (2, 3)
    for tri in f:
        a, b, c = v[tri].astype(np.float64)
        nrm = np.cross(b - a, c - a)
        assert nrm[0] > 0 and nrm[1] == 0 and nrm[2] == 0
    assert sorted(set(f.reshape(-1).tolist())) == [0, 1, 2, 3]
    # empty meshes: a dimension of 1, and a grid entirely inside
    assert R.marching_cubes(np.ones((1, 5, 5), np.float32), 0.5)[0].shape == (0, 3)
    v, f, n = R.marching_cubes(np.ones((3, 3, 3), np.float32), 0.5)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_reference_sphere_is_closed():
    x = np.linspace(-1, 1, 24, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    sig = (100 * np.maximum(0, 0.7 - np.sqrt(X * X + Y * Y + Z * Z))).astype(np.float32)
    st = np.float32(2) / np.float32(23)
    v, f, n = R.marching_cubes(sig, 10.0, (-1, -1, -1), (st, st, st))
    closed, chi, vol, area = R.mesh_stats(v, f)
    assert closed and chi == 2 and vol > 0
    assert abs(vol / (4 / 3 * np.pi * 0.6 ** 3) - 1) < 0.03


def _read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")[:-1]
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0" and header[-1] == "end_header"
    elems, cur = [], None
    for line in header[2:-1]:
        w = line.split()
        if w[0] == "element":
            cur = [w[1], int(w[2]), []]
            elems.append(cur)
        else:
            assert w[0] == "property"
            cur[2].append(tuple(w[1:]))
    (vn, V, vprops), (fn, F, fprops) = elems
    assert vn == "vertex" and fn == "face" and fprops == [("list", "uchar", "int", "vertex_indices")]
    types = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(p[1], types[p[0]]) for p in vprops])
    verts = np.frombuffer(data, vdt, V, end)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    faces = np.frombuffer(data, fdt, F, end + V * vdt.itemsize)
    assert end + V * vdt.itemsize + F * fdt.itemsize == len(data)
    return header, verts, faces


def test_write_ply_round_trip(pkg, tmp_path):
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    rgb = np.float32([[0, 0.5, 1], [1.2, -0.1, 0.499], [0.2, 0.3, 0.4], [0.998, 0.002, 0.5], [0, 0, 0], [1, 1, 1], [0.25, 0.75, 0.1]])
    f = np.int32([[0, 1, 2], [2, 3, 4], [4, 5, 6]])
    p = str(tmp_path / "m.ply")
    pkg.mesh.write_ply(p, v, f, normals=n, rgb=rgb)
    header, V, F = _read_ply(p)
    assert header == ["ply", "format binary_little_endian 1.0", "element vertex 7", "property float x", "property float y",
                      "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
                      "property uchar green", "property uchar blue", "element face 3", "property list uchar int vertex_indices",
                      "end_header"]
    assert np.array_equal(np.stack([V["x"], V["y"], V["z"]], 1), v)
    assert np.array_equal(np.stack([V["nx"], V["ny"], V["nz"]], 1), n)
    assert np.array_equal(np.stack([V["red"], V["green"], V["blue"]], 1), np.clip(np.rint(rgb.astype(np.float64) * 255), 0, 255))
    assert (F["n"] == 3).all() and np.array_equal(F["i"], f)
    pkg.mesh.write_ply(p, v, f)  # positions only
    header, V, F = _read_ply(p)
    assert V.dtype.names == ("x", "y", "z") and np.array_equal(F["i"], f)
    with pytest.raises(ValueError):
        pkg.mesh.write_ply(p, v, f, normals=n[:3])


def test_mesh_abi_declared_bound_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    declared = set(re.findall(r"\b(nerf_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    for name in MESH_SYMBOLS:
        assert name in declared and name in pkg._abi.EXPORTS and hasattr(lib, name), name


def test_mesh_ws_bytes(pkg):
    w = pkg._abi.mesh_ws_bytes
    n = w(64, 64, 64)
    assert n % 256 == 0 and 4 * 64 ** 3 <= n < 4 * 64 ** 3 + 4096
    assert w(512, 512, 512) >= 4 * 512 ** 3
    assert w(1, 5, 5) > 0 and w(2047, 1024, 1024) > w(1024, 1024, 1024)
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        with pytest.raises(pkg._abi.NerfHipError, match="positive"):
            w(*dims)
    with pytest.raises(pkg._abi.NerfHipError, match="2\\^31"):
        w(2048, 1024, 1024)


def test_mesh_calls_refuse_bad_arguments(pkg):
    L = pkg._abi.lib()
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = ctypes.c_void_p(1 << 20)  # (pointer values only: nothing is dereferenced before a refusal)

    def count(*dims, level=0.5, ws_bytes=1 << 30):
        return pkg._abi.check(L.nerf_hip_mesh_count(p, *dims, level, ws, ws_bytes, p, None))

    def emit(*dims, level=0.5, st=step, ws_bytes=1 << 30):
        return pkg._abi.check(L.nerf_hip_mesh_emit(p, *dims, lo, st, level, ws, ws_bytes, p, p, p, 4, 4, None))

    for call in (count, emit):
        for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            with pytest.raises(pkg._abi.NerfHipError, match="positive"):
                call(*dims)
        for dims in ((2048, 1024, 1024), (65536, 65536, 2)):
            with pytest.raises(pkg._abi.NerfHipError, match="2\\^31"):
                call(*dims)
        for lv in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(pkg._abi.NerfHipError, match="not finite"):
                call(4, 4, 4, level=lv)
        with pytest.raises(pkg._abi.NerfHipError, match="workspace"):
            call(4, 4, 4, ws_bytes=pkg._abi.mesh_ws_bytes(4, 4, 4) - 1)
    rc = L.nerf_hip_mesh_count(p, 4, 4, 4, 0.5, ws, 1 << 30, None, None)
    assert rc == -1 and "counts" in L.nerf_hip_last_error().decode()
    for bad in ([1, 0, 1], [1, 1, -1], [float("nan"), 1, 1]):
        with pytest.raises(pkg._abi.NerfHipError, match="step"):
            emit(4, 4, 4, st=pkg._abi.f32_array(bad))
    with pytest.raises(pkg._abi.NerfHipError, match="step"):
        emit(4, 1, 4, st=pkg._abi.f32_array([1, 1, 0]))
    # a zero step along a dimension of ONE point is no error (that dimension has no edges); it fails on the device check
    # or succeeds, never on the step
    rc = L.nerf_hip_mesh_emit(p, 4, 1, 4, lo, pkg._abi.f32_array([1, 0, 1]), 0.5, ws, 1 << 30, p, p, p, 4, 4, None)
    assert rc == 0 or "step" not in L.nerf_hip_last_error().decode()
    with pytest.raises(pkg._abi.NerfHipError, match="capacities"):
        pkg._abi.check(L.nerf_hip_mesh_emit(p, 4, 4, 4, lo, step, 0.5, ws, 1 << 30, p, p, p, -1, 4, None))
    with pytest.raises(pkg._abi.NerfHipError, match="null"):
        pkg._abi.check(L.nerf_hip_mesh_emit(p, 4, 4, 4, lo, step, 0.5, ws, 1 << 30, None, p, p, 4, 4, None))


def test_mesh_needs_a_device_tensor(pkg):
    import torch

    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)


def test_cli_parses_mesh_options(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    a = ap.parse_args(["--mesh", "256", "--mesh-level", "12.5", "--grid-bbox", "-1", "-1", "-1", "1", "1", "1"])
    assert a.mesh == 256 and a.mesh_level == 12.5 and a.grid_bbox == [-1.0] * 3 + [1.0] * 3
    d = ap.parse_args([])
    assert d.mesh is None and d.mesh_level == 50.0
