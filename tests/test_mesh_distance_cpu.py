"""CPU: the numpy restatement of the geometry evaluation (tests/distance_reference.py) against a plain-loop reading of
include/nerf_hip.h and, for the nearest points, against the O(N M) brute force; properties of the definitions; and the PLY reader
(mesh.read_ply) against mesh.write_ply, hand-written files and every refusal."""
import itertools

import numpy as np
import pytest

import distance_reference as D
import simplify_meshes as M
import smooth_reference as S

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


MESHES = {
    "blobs": lambda: M.blobs()[:2],
    "random": lambda: M.random_mesh()[:2],
    "fan": lambda: M.fan()[:2],
    "bad_input": lambda: M.bad_input()[:2],
    "patchwork": S.patchwork,
    "triangle": lambda: (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2]], np.int32)),
}


# ---- restatement against the plain loops ----

@pytest.mark.parametrize("name", ["patchwork", "triangle", "fan"])
def test_measure_restatement_equals_the_loops(name):
    v, f = MESHES[name]()
    f = f[:300]
    for lo, scale in (S.default_box(v), ((0.5, 0.25, 0.0), 0.5)):
        assert D.measure_raw(v, f, lo, scale) == D.measure_loops(v, f, lo, scale)


@pytest.mark.parametrize("name", ["patchwork", "triangle", "fan"])
def test_sampling_restatement_equals_the_loops(name):
    v, f = MESHES[name]()
    f = f[:200]
    lo, scale = S.default_box(v)
    for n, seed in ((1, 0), (37, 0), (37, 2 ** 32 - 1)):
        p, fid, W = D.sample_surface(v, f, n, seed, lo, scale)
        pl, fl, Wl = D.sample_loops(v, f, n, seed, lo, scale)
        assert W == Wl > 0 and np.array_equal(fid, fl) and np.array_equal(_bits(p), _bits(pl))
    i = np.arange(50)
    for s in range(3):
        assert np.array_equal(D.uniform(7, i, s), [D.uniform_loop(7, int(k), s) for k in i])
    assert not np.array_equal(D.uniform(7, i, 0), D.uniform(8, i, 0)) and not np.array_equal(D.uniform(7, i, 0), D.uniform(7, i, 1))
    r = D.uniform(3, np.arange(100000), 1)
    assert 0 < r.min() and r.max() < 1 and abs(r.mean() - 0.5) < 0.01


def test_nearest_restatement_equals_the_loops_and_the_definition():
    ref, q = D.cloud(70, 1).copy(), D.cloud(40, 2).copy()
    ref[5] = ref[60]            # an exact tie: the lower index wins
    ref[11, 1] = np.nan
    ref[12, 0] = np.inf
    q[3, 2] = -np.inf
    q[7] = ref[60]
    idx, d2 = D.nearest(ref, q)
    il, dl = D.nearest_loops(ref, q)
    assert np.array_equal(idx, il) and np.array_equal(d2.view(np.int64), dl.view(np.int64))
    assert idx[7] == 5 and d2[7] == 0 and idx[3] == -1 and np.isinf(d2[3]) and 11 not in idx and 12 not in idx
    idx, d2 = D.nearest(np.full((4, 3), np.nan, F32), q)
    assert (idx == -1).all() and np.isinf(d2).all()
    idx, d2 = D.nearest(np.zeros((0, 3), F32), q)
    assert (idx == -1).all() and len(D.nearest(ref, np.zeros((0, 3), F32))[0]) == 0


def test_stats_restatement_equals_the_loops():
    rng = np.random.default_rng(4)
    d2 = rng.random(500) ** 2
    d2[::50] = [np.inf, np.nan, -1.0, 100.0, 65.0, 0.0, 0.25, 1e-300, 63.9, 64.0]
    taus = (0.0, 0.5, 1.0, 8.0)
    a, b = D.distance_stats(d2, 1.0, taus), D.distance_stats_loops(d2, 1.0, taus)
    assert a == b and a[0] == 497 and a[3] == 2  # (100 and 65 are clamped; 64 is not)
    assert D.distance_stats(d2, 0.125, taus) == D.distance_stats_loops(d2, 0.125, taus)
    assert D.distance_stats([0.25, 0.25, 1.0], 1.0, (0.5,)) == [3, 2 * 2 ** 30, int(1.5 * 2 ** 30), 0, 2]  # d2 <= tau^2: <=, not <


# ---- properties of the definitions ----

@pytest.mark.parametrize("name", ["blobs", "random", "bad_input", "patchwork"])
def test_stratification_positions_and_faces_never_chosen(name):
    v, f = MESHES[name]()
    v, f = np.array(v), np.array(f)
    if name == "blobs":
        f[5] = [f[5, 0], f[5, 0], f[5, 2]]       # a repeated index
        v = np.concatenate((v, v[f[9, :1]]))     # a zero-area face on a duplicated vertex
        f[9, 1] = len(v) - 1
    # (bad_input has vertices at -1e30: its default box has scale 2^100, in which every other face has weight 0 -- W == 0)
    box = dict(lo=(0.0, 0.0, 0.0), scale=16.0) if name == "bad_input" else {}
    if name == "bad_input":
        assert D.sample_surface(v, f, 5)[2] == 0 and (D.sample_surface(v, f, 5)[1] == -1).all() and not D.sample_surface(v, f, 5)[0].any()
    w = D.weights(v, f, **box)
    W = int(w.sum())
    for n in (1, 100, 5000):
        p, fid, Wr = D.sample_surface(v, f, n, seed=3, **box)
        assert Wr == W and (fid >= 0).all()
        got = np.bincount(fid, minlength=len(f))
        want = n * w.astype(np.float64) / W
        assert np.abs(got - want).max() <= 2, (name, n, np.abs(got - want).max())
        assert not got[w == 0].any()  # zero-area, out-of-range and non-finite faces are never chosen
        # every sample lies in its face: barycentrics recomputed in fp64 from the stored point
        near = np.abs(v[f[fid]]).max((1, 2)) < 100  # (not the faces that reach out to 1e30: clamped into the box they weigh most)
        assert near.all() if name != "bad_input" else near.sum() >= n // 20
        p, fid = p[near], fid[near]
        a, b, c = (v[f[fid, k]].astype(np.float64) for k in range(3))
        e1, e2, d = b - a, c - a, p.astype(np.float64) - a
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        det = g11 * g22 - g12 * g12
        s = ((d * e1).sum(1) * g22 - (d * e2).sum(1) * g12) / det
        t = ((d * e2).sum(1) * g11 - (d * e1).sum(1) * g12) / det
        size = np.sqrt(np.maximum(g11, g22))
        tol = 2.0 ** -20  # (fp32 rounding of the point, 2^-24 of coordinates up to 32 against edges of about 1: far inside 2^-20)
        assert (s >= -tol).all() and (t >= -tol).all() and (s + t <= 1 + tol).all()
        resid = np.abs(d - s[:, None] * e1 - t[:, None] * e2).max(1)
        assert (resid <= 2.0 ** -18 * np.maximum(size, 1.0)).all()
    if name in ("bad_input", "patchwork", "blobs"):
        assert (w == 0).any()
    a, b = D.sample_surface(v, f, 200, seed=1, **box)[0], D.sample_surface(v, f, 200, seed=2, **box)[0]
    assert not np.array_equal(_bits(a), _bits(b))


def test_unit_cube_measures_are_exact():
    v, f = D.unit_cube()
    raw = D.measure_raw(v, f)
    assert raw[0] == 6 * 2 ** 40 and raw[1] == 6 * 2 ** 40 and raw[2:5] == [3 * 2 ** 40] * 3 and raw[5] == 12
    # in the mesh's units (mesh.measure_from_raw's arithmetic): exactly 6 and 1, the centroid the cube's centre
    assert raw[0] / 2.0 ** 40 == 6.0 and raw[1] / (6.0 * 2.0 ** 40) == 1.0
    flipped = D.measure_raw(v, f[:, ::-1])
    assert flipped[1] == -raw[1] and flipped[0] == raw[0]
    shifted = D.measure_raw(v * F32(2.0) + F32(3.0), f)  # a cube of side 2 at (3, 3, 3): its default box has scale 2
    assert shifted[:2] == [6 * 2 ** 40, 6 * 2 ** 40]


def test_sphere_volume_agrees_with_the_fp64_sum():
    v, f, _ = S.sphere32()
    lo, scale = S.default_box(v)
    raw = D.measure_raw(v, f)
    got = raw[1] / (6.0 * 2.0 ** 40) * float(scale) ** 3
    want = S.volume(v, f)
    # measure() is the same sum in box coordinates u = (p - lo) / scale (a translation leaves a closed mesh's volume alone), each
    # face's six-volume rounded to 2^-40: at most 2^-41 / 6 box volumes per face, plus the fp64 rounding of either sum -- terms of
    # up to |p|^3 = 32^3 each, 2^-50 relative with room to spare
    F = len(f)
    bound = F * (2.0 ** -41 / 6.0) * float(scale) ** 3 + F * 32.0 ** 3 * 2.0 ** -50
    print(f"sphere32: F {F}, scale {scale}, volume fixed point {got!r} fp64 {want!r}, difference {got - want:.3e}, bound {bound:.3e}")
    assert raw[5] == F and abs(got - want) <= bound and bound < 1e-6 * want
    area = raw[0] / 2.0 ** 40 * float(scale) ** 2
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    area64 = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(1)).sum()
    assert abs(area - area64) <= F * 2.0 ** -41 * float(scale) ** 2 + 1e-9


@pytest.mark.parametrize("delta", [0.25, 0.1])
def test_two_squares(delta):
    n = 400
    (va, fa), (vb, fb) = D.square(0.0, 3), D.square(delta, 2)
    pa, pb = D.sample_surface(va, fa, n, 0)[0], D.sample_surface(vb, fb, n, 1)[0]
    assert (pa[:, 2] == 0).all() and (pb[:, 2] == F32(delta)).all()
    d64 = np.float64(F32(delta))
    far = float(np.sqrt(d64 * d64 + 2.0))
    taus = (0.0, 0.5 * delta, float(np.nextafter(d64, 0)), float(np.nextafter(far, np.inf)), far * 2)
    r = D.chamfer(pa, pb, taus)
    assert (r["d_ab"] >= d64 * d64).all() and (r["d_ba"] >= d64 * d64).all()
    assert r["precision"][:3] == [0.0] * 3 == r["recall"][:3] and r["precision"][3:] == [1.0] * 2 == r["recall"][3:]
    assert r["raw_ab"][3] == 0 and r["raw_ba"][3] == 0 and r["unit"] == 1.0
    print(f"delta {delta}: mean a->b {r['mean_ab']:.6f} b->a {r['mean_ba']:.6f}")
    assert r["mean_ab"] >= delta * (1 - 1e-6) and r["mean_ba"] >= delta * (1 - 1e-6)


def test_default_unit_keeps_the_clamp_silent():
    a, b = D.cloud(300, 5, 3.0), D.cloud(200, 6, 0.01) + F32(2.9)
    r = D.chamfer(a, b, ())
    assert r["unit"] == 4.0 and r["raw_ab"][3] == 0 and r["raw_ba"][3] == 0
    assert D.chamfer(a, b, (), unit=2.0 ** -6)["raw_ab"][3] > 0  # a unit chosen too small is reported


# ---- the grid's sizing rule (host arithmetic: no device) ----

def test_grid_rule(pkg):
    rule = pkg.mesh.grid_rule
    for lo, hi, m in (((0, 0, 0), (1, 1, 1), 1000), ((0, 0, 0), (1, 1e-3, 1e-3), 1000), ((-5, 2, 1), (-5, 2, 1), 10), ((0, 0, 0), (1, 0, 0), 5),
                      ((0, 0, 0), (0, 7, 7), 1), ((-3e38, -3e38, -3e38), (3e38, 3e38, 3e38), 3), ((0, 0, 0), (1e-44, 0, 1e-44), 50),
                      ((0, 0, 0), (1, 1, 1), 10 ** 9)):
        glo, cell, dims = rule(np.asarray(lo, F32), np.asarray(hi, F32), m)
        ext = np.asarray(hi, F32).astype(np.float64) - np.asarray(lo, F32).astype(np.float64)
        assert np.isfinite(cell) and cell > 0 and all(d >= 1 for d in dims) and dims[0] * dims[1] * dims[2] <= 2 * m + 8 < 2 ** 31
        assert all(d == 1 for d, e in zip(dims, ext) if e == 0)  # one cell along an axis of zero extent
        assert np.array_equal(glo, np.asarray(lo, F32))
    assert rule(np.zeros(3, F32), np.zeros(3, F32), 0)[2] == (1, 1, 1)
    assert rule(np.zeros(3, F32), np.ones(3, F32), 1000)[2] == (10, 10, 10)


# ---- PLY ----

def test_read_ply_round_trips_write_ply(pkg, tmp_path):
    v, f, n = M.random_mesh()
    v = v.copy()
    v[3, 1], v[4, 0] = np.nan, -np.inf
    rgb = np.random.default_rng(2).random((len(v), 3)).astype(F32) * F32(1.2) - F32(0.1)
    for with_n, with_c in itertools.product((False, True), repeat=2):
        path = tmp_path / f"m{int(with_n)}{int(with_c)}.ply"
        pkg.mesh.write_ply(path, v, f, n if with_n else None, rgb if with_c else None)
        gv, gf, gn, gc = pkg.mesh.read_ply(path)
        assert gv.dtype == F32 and gf.dtype == np.int32 and np.array_equal(_bits(gv), _bits(v)) and np.array_equal(gf, f)
        assert (gn is None) == (not with_n) and (gc is None) == (not with_c)
        if with_n:
            assert np.array_equal(_bits(gn), _bits(n))
        if with_c:
            assert gc.dtype == np.uint8 and np.array_equal(gc, np.clip(np.rint(rgb.astype(np.float64) * 255.0), 0, 255).astype(np.uint8))
    pkg.mesh.write_ply(tmp_path / "e.ply", np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))
    gv, gf, gn, gc = pkg.mesh.read_ply(tmp_path / "e.ply")
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gn is None and gc is None


ASCII = """ply
format ascii 1.0
comment a hand-written tetrahedron
element vertex 4
property float x
property float y
property float z
element face 4
property list uchar int vertex_indices
end_header
0 0 0
1 0 0
0 1 0
0 0 1.5
3 0 2 1
3 0 1 3
3 1 2 3
3 0 3 2
"""

ASCII_EXTRA = """ply
format ascii 1.0
obj_info made by hand
element vertex 3
property double x
property float confidence
property float y
property uchar red
property uchar green
property uchar blue
property float z
property short label
element face 1
property list uint8 uint32 vertex_index
end_header
0.5 0.9 1 255 0 7 2 -3
1 0.8 0 1 2 3 0.25 4
0 0.7 0 9 9 9 1e-3 5
3 2 1 0
"""


def test_read_ply_hand_written_files(pkg, tmp_path):
    (tmp_path / "a.ply").write_text(ASCII)
    v, f, n, c = pkg.mesh.read_ply(tmp_path / "a.ply")
    assert np.array_equal(v, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], F32)) and n is None and c is None
    assert np.array_equal(f, [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]) and f.dtype == np.int32
    (tmp_path / "b.ply").write_text(ASCII_EXTRA)
    v, f, n, c = pkg.mesh.read_ply(tmp_path / "b.ply")
    assert np.array_equal(v, np.array([[0.5, 1, 2], [1, 0, 0.25], [0, 0, 1e-3]], F32)) and np.array_equal(f, [[2, 1, 0]]) and n is None
    assert np.array_equal(c, [[255, 0, 7], [1, 2, 3], [9, 9, 9]]) and c.dtype == np.uint8
    # the same file in binary, the skipped properties of other sizes between the coordinates
    rec = np.zeros(3, np.dtype([("x", "<f8"), ("confidence", "<f4"), ("y", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                                ("z", "<f4"), ("label", "<i2")]))
    rec["x"], rec["y"], rec["z"], rec["red"] = v[:, 0], v[:, 1], v[:, 2], c[:, 0]
    rec["green"], rec["blue"] = c[:, 1], c[:, 2]
    head = ASCII_EXTRA[:ASCII_EXTRA.index("end_header") + 11].replace("format ascii 1.0", "format binary_little_endian 1.0").replace("\n", "\r\n")
    face = np.array([(3, [2, 1, 0])], np.dtype([("n", "u1"), ("i", "<u4", (3,))]))
    (tmp_path / "c.ply").write_bytes(head.encode() + rec.tobytes() + face.tobytes())
    v2, f2, _, c2 = pkg.mesh.read_ply(tmp_path / "c.ply")
    assert np.array_equal(_bits(v2), _bits(v)) and np.array_equal(f2, f) and np.array_equal(c2, c)


@pytest.mark.parametrize("old,new,names", [
    ("format ascii 1.0", "format binary_big_endian 1.0", "binary_big_endian"),
    ("format ascii 1.0", "format ascii 2.0", "ascii 2.0"),
    ("element face 4", "element edge 4", "element edge 4"),
    ("property float z", "property list uchar float z", "list uchar float z"),
    ("property float z", "property quad z", "property quad z"),
    ("property list uchar int vertex_indices", "property list float int vertex_indices", "list float int"),
    ("property list uchar int vertex_indices", "property int vertex_indices", "property int vertex_indices"),
    ("end_header", "property list uchar int texcoord\nend_header", "texcoord"),
    ("end_header", "element material 0\nend_header", "element material 0"),
    ("comment a hand-written tetrahedron", "texture file.png", "texture file.png"),
    ("element vertex 4", "element vertex four", "element vertex four"),
])
def test_read_ply_refuses_and_names_the_line(pkg, tmp_path, old, new, names):
    assert old in ASCII
    (tmp_path / "bad.ply").write_text(ASCII.replace(old, new))
    with pytest.raises(ValueError, match=names):
        pkg.mesh.read_ply(tmp_path / "bad.ply")


def test_read_ply_refuses_other_bodies(pkg, tmp_path):
    p = tmp_path / "bad.ply"
    cases = {
        "only triangles": ASCII.replace("3 0 2 1\n", "4 0 2 1 3\n"),
        "x, y and z": ASCII.replace("property float z\n", "property float w\n"),
        "not a PLY": ASCII.replace("ply\n", "plx\n", 1),
        "no 'format'": ASCII.replace("format ascii 1.0\n", ""),
        "ends after 3 of 4": ASCII.replace("3 0 3 2\n", ""),
        "the 4 vertices need": ASCII[:ASCII.index("end_header") + 11] + "0 0 0\n",
        "not a number": ASCII.replace("0 0 1.5", "0 0 z"),
        "'element vertex' and 'element face'": ASCII.replace("element face 4\nproperty list uchar int vertex_indices\n", ""),
    }
    for match, text in cases.items():
        p.write_text(text)
        with pytest.raises(ValueError, match=match):
            pkg.mesh.read_ply(p)
    v, f, n = M.random_mesh()
    pkg.mesh.write_ply(p, v, f)
    data = p.read_bytes()
    p.write_bytes(data[:-7])
    with pytest.raises(ValueError, match="ends after"):
        pkg.mesh.read_ply(p)
    quad = np.array([(4, [0, 1, 2])], np.dtype([("n", "u1"), ("i", "<i4", (3,))])).tobytes()
    p.write_bytes(data[:len(data) - 13 * len(f) + 13 * 5] + quad + data[len(data) - 13 * len(f) + 13 * 6:])
    with pytest.raises(ValueError, match="face 5 has 4 indices"):
        pkg.mesh.read_ply(p)
