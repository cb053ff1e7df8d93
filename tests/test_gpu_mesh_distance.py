"""GPU: geometry evaluation on the device (nerf_hip_mesh_measure, nerf_hip_mesh_sample, nerf_hip_points_grid_build,
nerf_hip_points_nearest, nerf_hip_distance_stats; mesh.measure / sample_surface / nearest / chamfer / compare;
NeRFRunner.extract_mesh(compare=)) against the numpy restatement in tests/distance_reference.py.  Everything is exact equality:
positions and distances as bits, indices, counts and fixed-point sums as integers."""
import ctypes
import glob
import json

import numpy as np
import pytest
import torch

import distance_reference as D
import simplify_meshes as M
import smooth_reference as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F32).view(np.int32)


def _bits64(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64).view(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the inputs are read-only)


def _mesh(pkg, dev, v, f):
    return pkg.mesh.Mesh(_t(np.asarray(v, dtype=F32), dev), _t(np.asarray(f, dtype=np.int32), dev), None, None)


TRIANGLE = (np.array([[0.5, 0.25, 0.0], [3.0, 0.5, 1.0], [1.0, 2.5, -1.0]], F32), np.array([[0, 1, 2]], np.int32))
MESHES = {
    "blobs": lambda: M.blobs()[:2],
    "random": lambda: M.random_mesh()[:2],
    "fan": lambda: M.fan()[:2],
    "bad_input": lambda: M.bad_input()[:2],
    "triangle": lambda: TRIANGLE,
}
# (bad_input reaches out to -1e30: in its default box, of scale 2^100, no other face has any weight -- see the sampling test)
SAMPLE_BOX = {"bad_input": ((0.0, 0.0, 0.0), 16.0)}
SMALL_BOX = {"blobs": ((8.0, 4.0, 9.0), 4.0), "random": ((5.0, 6.0, 4.0), 2.0), "fan": ((1.0, 0.3, 0.2), 0.25),
             "bad_input": ((5.0, 6.0, 4.0), 2.0), "triangle": ((1.0, 0.5, 0.0), 0.5)}


# ---- (1) nearest points ----

def _check_nearest(pkg, dev, ref, q, grids=(None,)):
    want_i, want_d = D.nearest(ref, q)
    tr, tq = _t(np.asarray(ref, F32).reshape(-1, 3), dev), _t(np.asarray(q, F32).reshape(-1, 3), dev)
    for grid in grids:
        for sort in (True, False):
            idx, d2 = pkg.mesh.nearest(tr, tq, grid=grid, sort_queries=sort)
            assert idx.dtype == torch.int32 and d2.dtype == torch.float64 and tuple(idx.shape) == (len(q),) == tuple(d2.shape)
            assert np.array_equal(idx.cpu().numpy(), want_i), (grid, sort)
            assert np.array_equal(_bits64(d2), _bits64(want_d)), (grid, sort)
    assert np.array_equal(_bits(tr), _bits(np.asarray(ref, F32).reshape(-1, 3)))  # the inputs are unchanged
    return want_i, want_d


def test_nearest_random_cloud(pkg, dev):
    ref, q = D.cloud(5000, 11), D.cloud(3000, 12, 1.25) - F32(0.125)  # (just over two scan blocks each, odd; queries overhang the box)
    assert pkg._abi.lib() is not None and 5000 > 2 * 2048 and np.prod(pkg.mesh.grid_rule(ref.min(0), ref.max(0), 5000)[2]) > 2 * 2048
    _check_nearest(pkg, dev, ref, q)
    # the grid is an accelerator only: a grid that fits badly gives the same answer
    lo = ref.min(0)
    _check_nearest(pkg, dev, ref[:700], q[:300], grids=((lo, 1.0, (1, 1, 1)), (lo + F32(0.4), 0.05, (7, 3, 11)), (lo - F32(3.0), 0.01, (2, 500, 1)),
                                                       (lo, 3e-3, (300, 300, 20))))


def test_nearest_queries_far_outside(pkg, dev):
    ref = D.cloud(2000, 13)
    q = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            p = D.cloud(50, 14 + axis).copy() * F32(3.0) - F32(1.0)
            p[:, axis] = F32(0.5 + sign * 100.0) + p[:, axis]  # 100 box widths out, on every side
            q.append(p)
    q.append(np.array([[1e6, -1e6, 1e6], [-3e38, 3e38, 0.5], [0.5, 0.5, 1e30]], F32))
    _, d2 = _check_nearest(pkg, dev, ref, np.concatenate(q))
    assert d2.min() > 90.0 ** 2


def test_nearest_all_reference_points_equal(pkg, dev):
    ref = np.tile(np.array([[0.3, -1.5, 2.25]], F32), (500, 1))
    idx, _ = _check_nearest(pkg, dev, ref, D.cloud(200, 15, 4.0) - F32(2.0))
    assert (idx == 0).all()


def test_nearest_lattice_ties_go_to_the_lowest_index(pkg, dev):
    g = np.arange(9, dtype=F32)
    ref = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ref = ref[np.random.default_rng(3).permutation(len(ref))]  # (the lowest index is then no corner in particular)
    c = np.arange(8, dtype=F32) + F32(0.5)
    q = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    idx, d2 = _check_nearest(pkg, dev, ref, q)
    assert (d2 == 0.75).all()
    corners = (np.abs(ref[None, :, :].astype(np.float64) - q[:, None, :]) == 0.5).all(2)
    assert (corners.sum(1) == 8).all() and np.array_equal(idx, corners.argmax(1))


def test_nearest_coplanar_and_collinear_references(pkg, dev):
    q = D.cloud(400, 16, 2.0) - F32(0.5)
    plane = D.cloud(3000, 17).copy()
    plane[:, 1] = F32(0.375)
    _check_nearest(pkg, dev, plane, q)
    line = np.zeros((2500, 3), F32)
    line[:, 2] = D.cloud(2500, 18)[:, 0]
    line[:, 0] = F32(-2.0)
    _check_nearest(pkg, dev, line, q)
    assert pkg.mesh.nearest_grid(_t(plane, dev))[2][1] == 1 and pkg.mesh.nearest_grid(_t(line, dev))[2][:2] == (1, 1)


def test_nearest_one_crowded_cell_and_outliers(pkg, dev):
    rng = np.random.default_rng(19)
    crowd = (F32(0.5) + rng.random((4750, 3), dtype=F32) * F32(1e-4)).astype(F32)
    out = (rng.random((250, 3), dtype=F32) * F32(64.0) - F32(32.0)).astype(F32)
    ref = np.concatenate((crowd, out))[rng.permutation(5000)]
    q = np.concatenate(((rng.random((600, 3), dtype=F32) * F32(64.0) - F32(32.0)).astype(F32), crowd[:100] + F32(2e-5)))
    lo, cell, dims = pkg.mesh.nearest_grid(_t(ref, dev))
    _, counts = pkg.ops.points_grid(_t(ref, dev), lo.tolist(), float(cell), dims)
    fin, most = counts.cpu().tolist()
    assert fin == 5000 and most >= 4750 and np.prod(dims) > 4000  # 95 % of the points in one cell of thousands: long walks over empty cells
    _check_nearest(pkg, dev, ref, q)


# one workgroup of the cell scan (2048 cells) less one, exactly one, one more; 1024 * 2048 + 1: the first size at which a thread of the
# scan of the workgroups' totals takes a run of two
SCAN_EDGES = (2047, 2048, 2049, 1024 * 2048 + 1)


@pytest.mark.parametrize("ncell,axis", [(2047, 0), (2048, 2), (2049, 0), (2049, 2), (1024 * 2048 + 1, 2)])
def test_nearest_grids_at_the_scan_edges(pkg, dev, ncell, axis):
    """Explicit grids of ncell cells in a row along one axis: the first cell, the last, and the cells on both sides of the first
    workgroup's end hold points; the last cell is the fullest."""
    cell = F32(1.0) / F32(ncell)
    dims = [1, 1, 1]
    dims[axis] = ncell
    rng = np.random.default_rng(ncell + axis)
    ref, q = D.cloud(300, 61 + axis).copy(), D.cloud(200, 63 + axis).copy()
    at = [k for k in (0, 2046, 2047, 2048, ncell - 2, ncell - 1) if k < ncell] + [ncell - 1] * 6
    ref[:len(at), axis] = ((np.array(at, np.float64) + 0.5) * np.float64(cell)).astype(F32)
    ref[len(at), 1] = np.nan  # one row that is not finite
    ref = ref[rng.permutation(len(ref))]
    q[:len(at), axis] = ref[:len(at), axis][::-1]
    fin = np.isfinite(ref).all(1)
    k = np.clip(np.floor((ref[fin, axis].astype(np.float64) - 0.0) / np.float64(cell)), 0, ncell - 1).astype(np.int64)
    per = np.bincount(k, minlength=ncell)
    assert per[0] >= 1 and per[ncell - 1] == per.max() >= 7 and all(per[c] >= 1 for c in (2046, 2047, 2048) if c < ncell)
    want_i, want_d = D.nearest(ref, q)
    tr, tq = _t(ref, dev), _t(q, dev)
    ws, counts = pkg.ops.points_grid(tr, (0.0, 0.0, 0.0), float(cell), dims, n_query=len(q))
    assert counts.cpu().tolist() == [int(fin.sum()), int(per.max())]
    for sort in (False, True):
        idx, d2 = pkg.ops.points_nearest(tq, len(ref), (0.0, 0.0, 0.0), float(cell), dims, ws, sort_queries=sort)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(_bits64(d2), _bits64(want_d)), sort


def test_nearest_rows_that_are_not_finite(pkg, dev):
    ref, q = D.cloud(3000, 20).copy(), D.cloud(1000, 21).copy()
    rng = np.random.default_rng(22)
    for arr, k in ((ref, 300), (q, 100)):
        rows = rng.choice(len(arr), k, replace=False)
        arr[rows, rng.integers(0, 3, k)] = np.resize(np.array([np.nan, np.inf, -np.inf], F32), k)
    q[5] = ref[np.flatnonzero(np.isfinite(ref).all(1))[7]]
    idx, d2 = _check_nearest(pkg, dev, ref, q)
    bad_q = ~np.isfinite(q).all(1)
    assert (idx[bad_q] == -1).all() and np.isinf(d2[bad_q]).all() and (idx[~bad_q] >= 0).all() and np.isfinite(ref[idx[~bad_q]]).all()
    idx, d2 = _check_nearest(pkg, dev, np.full((70, 3), np.nan, F32), q[:50])  # no finite reference point at all
    assert (idx == -1).all() and np.isinf(d2).all()


def test_nearest_edge_sizes(pkg, dev):
    q = D.cloud(300, 23)
    idx, _ = _check_nearest(pkg, dev, np.array([[0.1, 0.2, 0.3]], F32), q)
    assert (idx == 0).all()
    idx, d2 = _check_nearest(pkg, dev, np.zeros((0, 3), F32), q)
    assert (idx == -1).all() and np.isinf(d2).all()
    idx, d2 = _check_nearest(pkg, dev, D.cloud(100, 24), np.zeros((0, 3), F32))
    assert idx.shape == (0,) and d2.shape == (0,)
    _check_nearest(pkg, dev, np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.nearest(torch.zeros(4, 3), torch.zeros(4, 3))


# ---- (2) surface samples ----

@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "triangle"])
def test_sample_surface(pkg, dev, name):
    v, f = MESHES[name]()
    m = _mesh(pkg, dev, v, f)
    lo, scale = SAMPLE_BOX.get(name, (None, None))
    first = {}
    for n in (1, 2049, 10000):
        for seed in (0, 77):
            want_p, want_f, W = D.sample_surface(v, f, n, seed, lo, scale)
            p, fid = pkg.mesh.sample_surface(m, n, seed, lo, scale)
            assert p.dtype == torch.float32 and fid.dtype == torch.int32 and tuple(p.shape) == (n, 3) and tuple(fid.shape) == (n,)
            assert np.array_equal(fid.cpu().numpy(), want_f) and np.array_equal(_bits(p), _bits(want_p)) and W > 0 and (want_f >= 0).all()
            first[(n, seed)] = _bits(p)
    assert not np.array_equal(first[(10000, 0)], first[(10000, 77)])  # two seeds give different bits
    p, fid = pkg.mesh.sample_surface(m, 0, 0, lo, scale)
    assert tuple(p.shape) == (0, 3) and tuple(fid.shape) == (0,)
    assert np.array_equal(_bits(m.verts), _bits(v)) and np.array_equal(m.faces.cpu().numpy(), f)
    if name == "blobs":
        assert len(f) == 2052  # one over a scan block


def _scan_edge_mesh(F):
    """300 random vertices, F faces of three distinct random corners; one face in ten, and faces on both sides of the first workgroup's
    end, repeat a corner and so weigh nothing"""
    rng = np.random.default_rng(F)
    V = 300
    a, o1, d = rng.integers(0, V, F), rng.integers(1, V, F), rng.integers(1, V - 1, F)
    o2 = (o1 - 1 + d) % (V - 1) + 1  # in [1, V), and never o1
    f = np.stack((a, (a + o1) % V, (a + o2) % V), axis=1).astype(np.int32)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    flat = rng.random(F) < 0.1
    flat[[k for k in (0, 2045, 2047, 2049, 2050) if k < F]] = True
    flat[[k for k in (2046, 2048) if k < F]] = False
    f[flat, 1] = f[flat, 0]
    return D.cloud(V, 71), f


@pytest.mark.parametrize("F", SCAN_EDGES)
def test_sample_surface_at_the_scan_edges(pkg, dev, F):
    """The scan of the weights at its partition edges (the reference at F = 2^21 + 1 takes about 3 s of numpy)."""
    v, f = _scan_edge_mesh(F)
    # the first seed whose REFERENCE samples reach a face of the second workgroup (F = 2049 has one such face with a weight, 2048)
    for seed in range(7, 64):
        want_p, want_f, W = D.sample_surface(v, f, 1000, seed)
        if F <= 2048 or want_f.max() >= 2048:
            break
    w = D.weights(v, f[:2051])
    assert w[0] == 0 and w[2045] == 0 and w[2046] > 0 and (F <= 2047 or w[2047] == 0) and (F <= 2048 or w[2048] > 0)
    assert W > 0 and (want_f >= 0).all() and (F <= 2048 or want_f.max() >= 2048)
    m = _mesh(pkg, dev, v, f)
    lo, scale = S.default_box(v)
    assert int(pkg.ops.mesh_sample(m.verts, m.faces, 1000, seed, lo.tolist(), float(scale))[2].cpu()) == W  # the scan's grand total
    p, fid = pkg.mesh.sample_surface(m, 1000, seed)
    assert np.array_equal(fid.cpu().numpy(), want_f) and np.array_equal(_bits(p), _bits(want_p))


def test_sample_surface_without_area(pkg, dev):
    v, f = MESHES["random"]()
    none = np.zeros((0, 3), np.int32)
    with pytest.raises(ValueError, match="no area"):
        pkg.mesh.sample_surface(_mesh(pkg, dev, v, none), 10)  # F = 0
    with pytest.raises(ValueError, match="no area"):
        pkg.mesh.sample_surface(_mesh(pkg, dev, np.zeros((0, 3), F32), none), 10)
    flat = np.zeros_like(v)
    with pytest.raises(ValueError, match="no area"):
        pkg.mesh.sample_surface(_mesh(pkg, dev, flat, f), 10)
    bv, bf = MESHES["bad_input"]()  # its default box (scale 2^100) leaves no face a weight: every face id -1, every point 0
    m = _mesh(pkg, dev, bv, bf)
    lo, scale = pkg.mesh.smooth_box(m.verts)
    assert scale == F32(2.0 ** 100) and D.sample_surface(bv, bf, 5)[2] == 0
    p, fid, info = pkg.ops.mesh_sample(m.verts, m.faces, 3000, 0, lo.tolist(), float(scale))
    assert int(info.cpu()) == 0 and (fid == -1).all() and not p.any()
    for bad in (dict(n=-1), dict(n=2 ** 31), dict(n=1.5), dict(n=5, seed=-1), dict(n=5, seed=2 ** 32), dict(n=5, scale=0.0), dict(n=5, lo=(0, np.nan, 0))):
        with pytest.raises(ValueError):
            pkg.mesh.sample_surface(m, **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.sample_surface(pkg.mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), None, None), 4)


# ---- (3) measures ----

@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "triangle"])
def test_measure(pkg, dev, name):
    v, f = MESHES[name]()
    m = _mesh(pkg, dev, v, f)
    for lo, scale in ((None, None), SMALL_BOX[name]):
        want = D.measure_raw(v, f, lo, scale)
        got = pkg.mesh.measure(m, lo, scale)
        assert list(got.raw) == want and got.faces == want[5]
        blo, bscale = S.default_box(v, lo, scale)
        assert got.area == want[0] / 2.0 ** 40 * float(bscale) ** 2 and got.volume == want[1] / (6 * 2.0 ** 40) * float(bscale) ** 3
        if lo is not None:
            uc, fin = S.box_coords(v, lo, scale)
            assert (uc[fin] == 2.0).any() and (uc[fin] == -1.0).any()  # vertices clamp on both sides of this box
    if name == "bad_input":
        assert pkg.mesh.measure(m).faces < len(f) - 60  # faces with bad indices and with corners that are not finite take no part
    if name == "triangle":
        got = pkg.mesh.measure(m)
        a, b, c = v.astype(np.float64)
        assert abs(got.area - 0.5 * np.linalg.norm(np.cross(b - a, c - a))) < 1e-9 and np.allclose(got.centroid, (a + b + c) / 3, atol=1e-9)


def test_measure_cube_and_empty(pkg, dev):
    v, f = D.unit_cube()
    got = pkg.mesh.measure(_mesh(pkg, dev, v, f))
    assert got.area == 6.0 and got.volume == 1.0 and got.faces == 12 and np.array_equal(got.centroid, [0.5, 0.5, 0.5])
    got = pkg.mesh.measure(_mesh(pkg, dev, v * F32(2.0) + F32(3.0), f[:, ::-1]))
    assert got.area == 24.0 and got.volume == -8.0 and np.array_equal(got.centroid, [4.0, 4.0, 4.0])
    e = pkg.mesh.measure(_mesh(pkg, dev, np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)))
    assert e.raw == (0,) * 8 and e.area == 0 and np.isnan(e.centroid).all()
    assert pkg.mesh.measure(_mesh(pkg, dev, v, np.zeros((0, 3), np.int32))).raw == (0,) * 8
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.measure(pkg.mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), None, None))


# ---- (4) statistics and Chamfer ----

def test_distance_stats(pkg, dev):
    rng = np.random.default_rng(31)
    d2 = rng.random(5001) ** 2 * 3.0
    d2[::500] = [np.inf, np.nan, -1.0, 100.0, 65.0, 0.0, 0.25, 1e-300, 63.9, 64.0, 0.25]
    taus = (0.0, 0.5, float(np.sqrt(d2[7])), 1.0, 1.7320508, 8.0, 0.123, 1e-200)  # 0.5 * 0.5 == 0.25 exactly: <=, not <
    for unit in (1.0, 0.125, 3.0):
        got = pkg.ops.distance_stats(_t(d2, dev), unit, taus).cpu().tolist()
        assert got == D.distance_stats(d2, unit, taus)
    want = D.distance_stats(d2, 1.0, taus)
    counted = d2[np.isfinite(d2) & (d2 >= 0)]
    assert want[3] == 2 and want[4 + 1] == int((counted <= 0.25).sum()) >= 2 + int((counted < 0.25).sum())
    assert pkg.ops.distance_stats(_t(d2, dev), 1.0).cpu().tolist() == want[:4]
    assert pkg.ops.distance_stats(_t(np.zeros(0), dev), 1.0, (1.0,)).cpu().tolist() == [0] * 5


def test_chamfer(pkg, dev):
    g = np.arange(6, dtype=F32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    a = np.concatenate((D.cloud(1500, 32, 5.0), lattice))
    b = np.concatenate((D.cloud(1201, 33, 5.0), lattice + np.array([0, 0, 0.5], F32)))
    taus = (0.25, 0.5, 1.0)  # the lattice points sit exactly 0.5 from their partners
    want = D.chamfer(a, b, taus)
    got = pkg.mesh.chamfer(_t(a, dev), _t(b, dev), taus)
    for side, raw in (("a_to_b", want["raw_ab"]), ("b_to_a", want["raw_ba"])):
        s = got[side]
        assert [s["count"], s["clamped"], *s["within"]] == [raw[0], raw[3], *raw[4:]]
        assert s["mean"] == raw[1] / (raw[0] * 2.0 ** 30) * want["unit"] and s["rms"] == float(np.sqrt(raw[2] / (raw[0] * 2.0 ** 30))) * want["unit"]
    assert got["unit"] == want["unit"] == 8.0 and got["clamped"] == 0
    assert got["precision"] == want["precision"] and got["recall"] == want["recall"] and got["chamfer"] == 0.5 * (want["mean_ab"] + want["mean_ba"])
    ties = int((want["d_ab"] == 0.25).sum())  # the distances that fall exactly on tau = 0.5 count
    assert ties >= 10 and got["a_to_b"]["within"][1] == int((want["d_ab"] < 0.25).sum()) + ties
    p, r = got["precision"][1], got["recall"][1]
    assert got["fscore"][1] == 2 * p * r / (p + r)
    tiny = pkg.mesh.chamfer(_t(a, dev), _t(b, dev), taus, unit=2.0 ** -4)
    raw = D.chamfer(a, b, taus, unit=2.0 ** -4)
    assert tiny["clamped"] == raw["raw_ab"][3] + raw["raw_ba"][3] > 0  # a unit too small is reported, never hidden
    for bad in (dict(unit=0.0), dict(unit=np.nan), dict(unit=1e200), dict(thresholds=(np.nan,)), dict(thresholds=(-1.0,)), dict(thresholds=(1.0,) * 9)):
        with pytest.raises(ValueError):
            pkg.mesh.chamfer(_t(a, dev), _t(b, dev), **bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.chamfer(torch.zeros(4, 3), torch.zeros(4, 3))


# ---- (5) determinism ----

def test_two_runs_give_identical_bytes(pkg, dev):
    v, f = MESHES["random"]()
    m = _mesh(pkg, dev, v, f)
    ref, q = _t(D.cloud(5000, 41), dev), _t(D.cloud(3000, 42), dev)
    runs = []
    for _ in range(2):
        p, fid = pkg.mesh.sample_surface(m, 10000, 5)
        i1, d1 = pkg.mesh.nearest(ref, q)
        i2, d2 = pkg.mesh.nearest(ref, q, sort_queries=False)
        c = pkg.mesh.chamfer(q, ref, (0.01, 0.05))
        runs.append((p.view(torch.int32), fid, i1, d1.view(torch.int64), i2, d2.view(torch.int64), pkg.mesh.measure(m).raw, c))
    for x, y in zip(*runs):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
    assert torch.equal(runs[0][2], runs[0][4]) and torch.equal(runs[0][3], runs[0][5])  # sorted and unsorted queries agree


# ---- (6) guard regions behind every output and the workspace ----

GUARD = 4096


def _raw_sample(pkg, dev, m, lo, scale, n, seed, cap):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F = int(m.verts.shape[0]), int(m.faces.shape[0])
    nws = pkg._abi.mesh_sample_ws_bytes(F)
    ws = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    pts = torch.full((cap + GUARD, 3), 7.25, device=dev)
    fid = torch.full((cap + GUARD,), -9, dtype=torch.int32, device=dev)
    info = torch.full((1 + 8,), -5, dtype=torch.int64, device=dev)
    out = torch.full((8 + 8,), -5, dtype=torch.int64, device=dev)
    lo3 = pkg._abi.f32_array(lo)
    pkg._abi.check(L.nerf_hip_mesh_sample(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, float(scale), n, seed, ws.data_ptr(), nws,
                                          pts.data_ptr(), fid.data_ptr(), cap, info.data_ptr(), st))
    pkg._abi.check(L.nerf_hip_mesh_measure(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, float(scale), out.data_ptr(), st))
    torch.cuda.synchronize()
    assert (ws[nws:] == 0x5A).all() and (info[1:] == -5).all() and (out[8:] == -5).all()
    return pts, fid, int(info[0]), out[:8].tolist()


def _raw_nearest(pkg, dev, ref, q, grid, cap, sort):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    lo, cell, dims = grid
    Mr, N = int(ref.shape[0]), int(q.shape[0])
    nws = pkg._abi.points_nearest_ws_bytes(Mr, N, dims)
    ws = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((2 + 8,), -5, dtype=torch.int64, device=dev)
    idx = torch.full((cap + GUARD,), -9, dtype=torch.int32, device=dev)
    d2 = torch.full((cap + GUARD,), 7.25, dtype=torch.float64, device=dev)
    lo3, dims3 = pkg._abi.f32_array(lo), pkg._abi.i32_array(dims)
    pkg._abi.check(L.nerf_hip_points_grid_build(ref.data_ptr(), Mr, lo3, float(cell), dims3, ws.data_ptr(), nws, counts.data_ptr(), st))
    pkg._abi.check(L.nerf_hip_points_nearest(q.data_ptr(), Mr, N, lo3, float(cell), dims3, ws.data_ptr(), nws, int(sort), idx.data_ptr(),
                                             d2.data_ptr(), cap, st))
    stats = torch.full((4 + 2 + 8,), -5, dtype=torch.int64, device=dev)
    tau = (ctypes.c_double * 2)(0.01, 0.05)
    pkg._abi.check(L.nerf_hip_distance_stats(d2.data_ptr(), min(cap, N), 1.0, tau, 2, stats.data_ptr(), st))
    torch.cuda.synchronize()
    assert (ws[nws:] == 0x5A).all() and (counts[2:] == -5).all() and (stats[6:] == -5).all()
    return idx, d2, counts[:2].tolist(), stats[:6].tolist()


def test_outputs_stay_inside_their_capacities(pkg, dev):
    v, f = MESHES["bad_input"]()
    m = _mesh(pkg, dev, v, f)
    lo, scale = SAMPLE_BOX["bad_input"]
    n = 3001
    want_p, want_f, W = D.sample_surface(v, f, n, 9, lo, scale)
    want_m = D.measure_raw(v, f, lo, scale)
    ref, q = D.cloud(3000, 51).copy(), D.cloud(n, 52).copy()
    ref[::97, 1] = np.nan
    q[::89, 0] = np.inf
    want_i, want_d = D.nearest(ref, q)
    tr, tq = _t(ref, dev), _t(q, dev)
    grid = pkg.mesh.nearest_grid(tr)
    for cap in (n, n // 2, 0, n - 1, n + 100):
        k = min(cap, n)
        pts, fid, Wg, out = _raw_sample(pkg, dev, m, lo, scale, n, 9, cap)
        assert Wg == W and out == want_m and (pts[k:] == 7.25).all() and (fid[k:] == -9).all()
        assert np.array_equal(_bits(pts[:k]), _bits(want_p[:k])) and np.array_equal(fid[:k].cpu().numpy(), want_f[:k])
        for sort in (True, False):
            idx, d2, counts, stats = _raw_nearest(pkg, dev, tr, tq, grid, cap, sort)
            assert counts[0] == int(np.isfinite(ref).all(1).sum()) and (idx[k:] == -9).all() and (d2[k:] == 7.25).all()
            assert np.array_equal(idx[:k].cpu().numpy(), want_i[:k]) and np.array_equal(_bits64(d2[:k]), _bits64(want_d[:k]))
            assert stats == D.distance_stats(want_d[:k], 1.0, (0.01, 0.05))
    assert np.array_equal(_bits(m.verts), _bits(v)) and np.array_equal(_bits(tr), _bits(ref)) and np.array_equal(_bits(tq), _bits(q))


# ---- (7) refusals on the host: nothing is launched ----

def test_host_refusals_launch_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F, N, Mr = 64, 32, 48, 40
    dims = (3, 2, 2)
    verts = torch.zeros(V, 3, device=dev)
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    pts = torch.zeros(max(N, Mr), 3, device=dev)
    need_s, need_g, need_n = pkg._abi.mesh_sample_ws_bytes(F), pkg._abi.points_nearest_ws_bytes(Mr, 0, dims), pkg._abi.points_nearest_ws_bytes(Mr, N, dims)
    assert need_g < need_n
    ws = torch.full((max(need_s, need_n),), 0x5A, dtype=torch.uint8, device=dev)
    out8 = torch.full((16,), -5, dtype=torch.int64, device=dev)
    opts = torch.full((N, 3), 2.5, device=dev)
    oidx = torch.full((N,), -9, dtype=torch.int32, device=dev)
    od2 = torch.full((N,), 2.5, dtype=torch.float64, device=dev)
    f3, i3 = pkg._abi.f32_array, pkg._abi.i32_array
    tau = (ctypes.c_double * 2)(0.5, 1.0)

    def measure(v=V, f=F, lo=(0, 0, 0), scale=1.0, vp=verts.data_ptr(), fp=faces.data_ptr(), op=out8.data_ptr()):
        return L.nerf_hip_mesh_measure(vp, fp, v, f, f3(lo), scale, op, st)

    def sample(v=V, f=F, lo=(0, 0, 0), scale=1.0, n=N, w=ws.data_ptr(), nbytes=need_s, vp=verts.data_ptr(), fp=faces.data_ptr(),
               pp=opts.data_ptr(), ip=oidx.data_ptr(), cap=N, op=out8.data_ptr()):
        return L.nerf_hip_mesh_sample(vp, fp, v, f, f3(lo), scale, n, 0, w, nbytes, pp, ip, cap, op, st)

    def build(m=Mr, lo=(0, 0, 0), cell=0.5, d=dims, w=ws.data_ptr(), nbytes=need_g, rp=pts.data_ptr(), cp=out8.data_ptr()):
        return L.nerf_hip_points_grid_build(rp, m, f3(lo), cell, i3(d), w, nbytes, cp, st)

    def near(m=Mr, n=N, lo=(0, 0, 0), cell=0.5, d=dims, w=ws.data_ptr(), nbytes=need_n, qp=pts.data_ptr(), ip=oidx.data_ptr(),
             dp=od2.data_ptr(), cap=N):
        return L.nerf_hip_points_nearest(qp, m, n, f3(lo), cell, i3(d), w, nbytes, 1, ip, dp, cap, st)

    def stats(n=N, unit=1.0, tp=tau, k=2, dp=od2.data_ptr(), op=out8.data_ptr()):
        return L.nerf_hip_distance_stats(dp, n, unit, tp, k, op, st)

    nan, inf = float("nan"), float("inf")
    for call in (measure, sample):
        assert call(v=-1) == -1 and call(f=1 << 31) == -1 and call(vp=None) == -1 and call(fp=None) == -1 and call(op=None) == -1
        assert call(op=out8.data_ptr() + 4) == -1 and call(lo=(0, nan, 0)) == -1 and call(lo=(inf, 0, 0)) == -1
        for scale in (0.0, -1.0, nan, inf):
            assert call(scale=scale) == -1
    assert sample(n=-1) == -1 and sample(n=1 << 31) == -1 and sample(cap=-1) == -1 and sample(pp=None) == -1 and sample(ip=None) == -1
    for call, need in ((sample, need_s), (build, need_g), (near, need_n)):
        assert call(w=None) == -1 and call(w=ws.data_ptr() + 4) == -1
        assert call(nbytes=need - 1) == -2  # one byte short
    for call in (build, near):
        assert call(m=-1) == -1 and call(m=1 << 31) == -1 and call(lo=(0, 0, nan)) == -1 and call(lo=(-inf, 0, 0)) == -1
        for cell in (0.0, -0.5, nan, inf):
            assert call(cell=cell) == -1
        assert call(d=(0, 1, 1)) == -1 and call(d=(1, -2, 1)) == -1 and call(d=(2048, 2048, 512)) == -1
    assert build(rp=None) == -1 and build(cp=None) == -1 and build(cp=out8.data_ptr() + 4) == -1
    assert near(n=-1) == -1 and near(qp=None) == -1 and near(ip=None) == -1 and near(dp=None) == -1 and near(dp=od2.data_ptr() + 4) == -1
    assert near(cap=-1) == -1
    for unit in (0.0, -1.0, nan, inf, 1e200, 1e-200):
        assert stats(unit=unit) == -1
    assert stats(n=-1) == -1 and stats(k=9) == -1 and stats(k=-1) == -1 and stats(tp=None) == -1 and stats(dp=None) == -1 and stats(op=None) == -1
    assert stats(tp=(ctypes.c_double * 2)(0.5, nan)) == -1 and stats(tp=(ctypes.c_double * 2)(-0.5, 1.0)) == -1
    for fn, args in ((pkg._abi.mesh_sample_ws_bytes, (-1,)), (pkg._abi.points_nearest_ws_bytes, (-1, 0, dims)),
                     (pkg._abi.points_nearest_ws_bytes, (4, 4, (0, 1, 1)))):
        with pytest.raises(pkg._abi.NerfHipError):
            fn(*args)
    torch.cuda.synchronize()
    untouched = lambda: ((out8 == -5).all() and (ws == 0x5A).all() and (opts == 2.5).all() and (oidx == -9).all() and (od2 == 2.5).all())
    assert untouched()
    assert measure() == 0  # and the good calls go through: every face repeats index 0, none takes part
    torch.cuda.synchronize()
    assert out8[:8].tolist() == [0] * 8 and (out8[8:] == -5).all()
    assert sample() == 0 and build() == 0 and near() == 0
    torch.cuda.synchronize()
    assert (oidx == 0).all() and (od2 == 0).all() and (opts == 0).all() and out8[:2].tolist() == [Mr, Mr]  # 40 equal points, one cell
    assert stats() == 0
    torch.cuda.synchronize()
    assert out8[:6].tolist() == [N, 0, 0, 0, N, N]


# ---- (8) inside extract_mesh ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


LO, HI, RES = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), 24


def test_compare_extracted_meshes(pkg, dev, model):
    """The extracted mesh against itself and against its simplify=2 version, on the smooth test's filtered mesh (min_faces=8).  A
    component whose area is below W / n gets one sample or none from either seed, so a mesh is at distance 0 from itself only up to
    its floaters: the unfiltered mesh of this model has 55 components, 50 of them of 1 to 4 faces on the box's faces, and at n = 200 000
    one of its samples (on a 4-face component that the other cloud misses) lies 0.1247 from the other cloud, more than the step of
    0.1065 -- precision 0.999995, F-score 0.9999975.  test_far_samples_sit_on_floaters holds the unfiltered mesh to exactly that."""
    level = float(model.density_grid(LO, HI, RES).median())
    kw = dict(normals="grid", color=False, min_faces=8)
    base = model.extract_mesh(LO, HI, RES, level, **kw)
    again = model.extract_mesh(LO, HI, RES, level, **kw)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base[:3], again[:3]))
    step = float(((np.asarray(HI, F32) - np.asarray(LO, F32)) / F32(RES - 1)).max())
    same = pkg.mesh.compare(base, base, thresholds=(step,))
    print(f"self: chamfer {same['chamfer']:.6f} step {step:.6f} F {same['fscore']} P {same['precision']} R {same['recall']} "
          f"area {same['measure_a'].area:.4f} faces {same['measure_a'].faces}")
    assert same["samples"] == 200_000 and same["clamped"] == 0 and same["measure_a"].raw == same["measure_b"].raw
    assert same["chamfer"] < step and same["fscore"] == [1.0] and same["precision"] == [1.0] == same["recall"]
    coarse = model.extract_mesh(LO, HI, RES, level, simplify=2, **kw)
    other = pkg.mesh.compare(coarse, base, thresholds=(step,))
    print(f"simplify=2: chamfer {other['chamfer']:.6f} F {other['fscore']} faces {other['measure_a'].faces} vs {other['measure_b'].faces}")
    assert other["chamfer"] > same["chamfer"] and other["measure_a"].faces < other["measure_b"].faces
    assert repr(pkg.mesh.compare(base, base, n=5000, seed=3)) == repr(pkg.mesh.compare(base, base, n=5000, seed=3))


def test_far_samples_sit_on_floaters(pkg, dev, model):
    """The unfiltered mesh against itself: its Chamfer distance is below one lattice step, and every sample that lies farther than
    one step from the other cloud sits on a component of fewer than 8 faces (see test_compare_extracted_meshes)."""
    level = float(model.density_grid(LO, HI, RES).median())
    base = model.extract_mesh(LO, HI, RES, level, normals="grid", color=False)
    step = float(((np.asarray(HI, F32) - np.asarray(LO, F32)) / F32(RES - 1)).max())
    same = pkg.mesh.compare(base, base, thresholds=(step,))
    comps = pkg.mesh.components(base.faces, len(base.verts))
    (pa, fa), (pb, fb) = pkg.mesh.sample_surface(base, 200_000, 0), pkg.mesh.sample_surface(base, 200_000, 1)
    far = 0
    for (p, f), q in (((pa, fa), pb), ((pb, fb), pa)):
        _, d2 = pkg.mesh.nearest(q, p)
        out = d2 > step * step
        far += int(out.sum())
        assert (comps.n_faces[comps.face_comp[f[out].long()].long()] < 8).all()
    print(f"unfiltered: chamfer {same['chamfer']:.6f} F {same['fscore']} P {same['precision']} R {same['recall']}, {far} samples beyond a step, "
          f"{len(comps.n_faces)} components, {int((comps.n_faces < 8).sum())} of fewer than 8 faces")
    assert same["chamfer"] < step and same["fscore"][0] >= 1 - far / 200_000 and far == round((2 - same["precision"][0] - same["recall"][0]) * 200_000)


def test_runner_compares_against_a_file(pkg, dev, tmp_path, capsys):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    level = float(np.median(run.density_grid(24, save=False)))
    plain = run.extract_mesh(24, level, save=True)
    files = glob.glob(rs + "*_mesh24.ply")
    assert len(files) == 1 and not glob.glob(rs + "*_mesh_eval.json") and not hasattr(run, "last_mesh_eval")
    assert "[MESH-EVAL]" not in capsys.readouterr().out
    step = 3.0 / 23
    got = run.extract_mesh(24, level, save=True, compare=files[0], compare_samples=20_000, compare_tau=(step, 2 * step))
    for a, b in zip(plain, got):  # the mesh is what it is without compare
        assert (a is None and b is None) or np.array_equal(a.view(np.int32) if a.dtype == F32 else a, b.view(np.int32) if b.dtype == F32 else b)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH-EVAL]")]
    out = glob.glob(rs + "*_mesh_eval.json")
    assert len(line) == 1 and len(out) == 1
    r = json.load(open(out[0]))
    assert r["truth"] == files[0] and r["samples"] == 20_000 and r["chamfer"] == run.last_mesh_eval["chamfer"] < step
    assert r["measure_a"] == r["measure_b"] and r["fscore"][1] == 1.0 and r["thresholds"] == [step, 2 * step]
    m2 = run.extract_mesh(24, level, save=False, compare=pkg.mesh.Mesh(plain.verts, plain.faces, None, None), compare_samples=20_000)
    assert run.last_mesh_eval["truth"] is None and run.last_mesh_eval["chamfer"] == r["chamfer"] and len(glob.glob(rs + "*_mesh_eval.json")) == 1
    assert np.array_equal(m2.faces, plain.faces)
