"""GPU: connected components of indexed meshes on the device (nerf_hip_mesh_cc_*, mesh.components / select_components /
filter_components, extract_mesh(min_faces=, keep_largest=)) against the numpy restatement in tests/cc_reference.py.  Everything is
exact equality: labels, counts, boxes (as bits), compacted meshes."""
import functools

import numpy as np
import pytest
import torch

import cc_reference as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(pkg, dev, faces, V, verts=None, ref=None):
    """components() of (faces, V, verts) equals the restatement; -> (Components, reference dict)."""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    ref = ref or R.components(faces, V, verts)
    c = pkg.mesh.components(torch.from_numpy(faces).to(dev), V, None if verts is None else torch.from_numpy(verts).to(dev))
    for name in ("vert_comp", "face_comp", "n_verts", "n_faces"):
        got = getattr(c, name)
        assert got.dtype == torch.int32 and got.device.type == "cuda", name
        assert np.array_equal(got.cpu().numpy(), ref[name]), name
    assert len(c.n_verts) == ref["C"]
    if verts is None:
        assert c.bbox_lo is None and c.bbox_hi is None
    else:
        assert c.bbox_lo.dtype == torch.float32 and tuple(c.bbox_lo.shape) == (ref["C"], 3)
        assert np.array_equal(_bits(c.bbox_lo.cpu().numpy()), _bits(ref["bbox_lo"]))
        assert np.array_equal(_bits(c.bbox_hi.cpu().numpy()), _bits(ref["bbox_hi"]))
    assert 1 <= c.rounds <= 64
    return c, ref


# ---- (1) blobs: three balls of different sizes and a one-cell island on a 24^3 grid ----

BALLS = (((6.3, 6.1, 6.4), 4.2), ((16.5, 7.2, 15.8), 5.3), ((9.1, 17.4, 12.2), 3.1))
ISLAND = (20, 20, 3)


@functools.lru_cache(maxsize=None)
def _blobs():
    """-> (sigma [24, 24, 24] fp32 with level 0, the reference marching-cubes mesh, the reference components)"""
    import mc_reference as MC

    g = np.arange(24, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    s = np.full((24, 24, 24), -1.0)
    for (cx, cy, cz), r in BALLS:
        s = np.maximum(s, r - np.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    s[ISLAND] = 0.75
    s = s.astype(np.float32)
    v, f, n = MC.marching_cubes(s, 0.0, (0, 0, 0), (1, 1, 1))
    return s, (v, f, n), R.components(f, len(v), v)


def _blob_mesh(pkg, dev):
    s, (rv, rf, _), ref = _blobs()
    v, f, n = pkg.mesh.marching_cubes(torch.from_numpy(s).to(dev), 0.0)
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(f.cpu().numpy(), rf)
    rgb = torch.stack([torch.arange(len(v), device=dev) % 7, torch.arange(len(v), device=dev) % 5, torch.arange(len(v), device=dev) % 3],
                      1).to(torch.float32) / 8
    return pkg.mesh.Mesh(v, f, n, rgb), ref


def test_blobs(pkg, dev):
    m, ref = _blob_mesh(pkg, dev)
    c, _ = _check(pkg, dev, m.faces.cpu().numpy(), len(m.verts), m.verts.cpu().numpy(), ref)
    assert ref["C"] == 4 and len(c.n_faces) == 4
    assert sorted(ref["n_faces"].tolist())[0] == 8 and sorted(ref["n_verts"].tolist())[0] == 6  # the island: an octahedron
    assert len(set(ref["n_faces"].tolist())) == 4
    isl = int(np.argmin(ref["n_faces"]))
    assert np.abs(c.bbox_lo[isl].cpu().numpy() - (np.float32(ISLAND) - 1)).max() < 1 and (c.bbox_hi[isl] > c.bbox_lo[isl]).all()


# ---- (2) a random field: V and F no multiple of a wave or a workgroup; at level 0.5 one giant component beside small ones, at
# level 0.9 hundreds of small ones, several ids in every wave of the counting kernels ----

@functools.lru_cache(maxsize=None)
def _random_mesh(level=0.5):
    import mc_reference as MC

    s = np.random.default_rng(16).random((16, 16, 16), dtype=np.float32)
    v, f, _ = MC.marching_cubes(s, level, (0, 0, 0), (1, 1, 1))
    return v, f, R.components(f, len(v), v)


@pytest.mark.parametrize("level", [0.5, 0.9])
def test_random_field(pkg, dev, level):
    v, f, ref = _random_mesh(level)
    assert len(v) % 64 and len(f) % 64 and len(v) > 256
    assert ref["C"] > (10 if level == 0.5 else 200)
    c, _ = _check(pkg, dev, f, len(v), v, ref)
    print(f"random 16^3 at {level}: V={len(v)} F={len(f)} C={ref['C']}, {c.rounds} rounds")


def test_labelling_is_deterministic(pkg, dev):
    v, f, _ = _random_mesh()
    ft, vt = torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
    a = pkg.mesh.components(ft, len(v), vt)
    b = pkg.mesh.components(ft, len(v), vt)
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- (3) triangle strips: long chains for the compress walk, many rounds ----

def _strip(n):
    i = np.arange(n - 2, dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1)


@pytest.mark.parametrize("n,permuted", [(65536, False), (4096, True), (65536, True)])
def test_triangle_strips(pkg, dev, n, permuted):
    faces = _strip(n)
    if permuted:
        faces = np.random.default_rng(0).permutation(n)[faces]
    c, ref = _check(pkg, dev, faces, n)
    assert ref["C"] == 1 and (c.vert_comp == 0).all() and (c.face_comp == 0).all()
    assert c.n_verts.tolist() == [n] and c.n_faces.tolist() == [n - 2]
    # (the synchronous restatement needs 2, 8 and 11 rounds: tests/test_mesh_components_cpu.py; the device's count may differ)
    print(f"strip n={n} permuted={permuted}: {c.rounds} rounds on the device")
    assert c.rounds <= 64


# ---- (4) edge cases ----

def test_edge_cases(pkg, dev):
    none = np.zeros((0, 3), np.int32)
    c, _ = _check(pkg, dev, none, 5, np.arange(15, dtype=np.float32).reshape(5, 3))  # F == 0: five isolated vertices
    assert c.n_verts.tolist() == [1] * 5 and c.n_faces.tolist() == [0] * 5 and c.rounds == 1
    assert torch.equal(c.bbox_lo, c.bbox_hi)
    c, _ = _check(pkg, dev, none, 0, np.zeros((0, 3), np.float32))  # V == 0
    assert len(c.n_verts) == 0 and len(c.vert_comp) == 0
    c, _ = _check(pkg, dev, [[0, 0, 0], [1, 2, 3]], 0)  # faces over no vertices: none takes part
    assert c.face_comp.tolist() == [-1, -1] and len(c.n_verts) == 0
    c, _ = _check(pkg, dev, [[0, 1, 2], [4, 5, 6]], 8)  # isolated vertices 3 and 7
    assert c.vert_comp.tolist() == [0, 0, 0, 1, 2, 2, 2, 3]
    c, _ = _check(pkg, dev, [[0, 1, 2], [2, 3, 4]], 5)  # the bow-tie: one shared vertex joins two triangles
    assert c.n_verts.tolist() == [5] and c.n_faces.tolist() == [2]
    _check(pkg, dev, [[5, 5, 2], [0, 1, 3], [0, 1, 3], [3, 1, 0], [4, 4, 4], [2, 6, 6]], 8)  # duplicate and degenerate faces
    verts = np.array([[1, 2, 3], [-1, np.nan, 5], [0.5, -2, np.inf], [-0.0, 1, np.nan], [0.0, 1, np.nan], [-0.0, 1, -np.inf],
                      [np.nan, np.nan, np.nan]], np.float32)
    c, _ = _check(pkg, dev, [[0, 1, 2], [3, 4, 5]], 7, verts)  # coordinates that are not finite are ignored; -0 counts as +0
    assert c.bbox_lo[2].tolist() == [np.inf] * 3 and c.bbox_hi[2].tolist() == [-np.inf] * 3


def test_out_of_range_faces_take_no_part(pkg, dev):
    V = 10
    faces = np.array([[0, 1, 2], [2, 3, -1], [3, 4, 5], [5, 6, 7], [7, 8, 9], [0, 9, V]], np.int32)  # one index -1, one index V
    verts = np.random.default_rng(3).random((V, 3), dtype=np.float32)
    c, ref = _check(pkg, dev, faces, V, verts)
    assert c.face_comp.tolist() == [0, -1, 1, 1, 1, -1] and c.n_faces.tolist() == [1, 3]
    m = pkg.mesh.Mesh(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), None, None)
    out = pkg.mesh.filter_components(m, c, torch.ones(2, dtype=torch.bool))
    rv, rf, _, _ = R.compact(verts, faces, ref["vert_comp"], ref["face_comp"], [True, True])
    assert out.normals is None and out.rgb is None
    assert np.array_equal(out.verts.cpu().numpy(), verts) and np.array_equal(out.faces.cpu().numpy(), rf) and len(rf) == 4
    # the same with huge and negative indices, in a mesh with more than one workgroup of faces
    rng = np.random.default_rng(4)
    V, F = 3000, 5000
    faces = np.sort(rng.integers(0, V, (F, 1), dtype=np.int64) // 50 * 50 + rng.integers(0, 50, (F, 3)), axis=0).astype(np.int32)
    bad = rng.choice(F, 40, replace=False)
    faces[bad, rng.integers(0, 3, 40)] = rng.choice(np.array([-1, V, V + 1, 2 ** 31 - 1, -2 ** 31, -V], np.int64), 40).astype(np.int32)
    c, ref = _check(pkg, dev, faces, V, rng.random((V, 3), dtype=np.float32))
    assert (c.face_comp[torch.from_numpy(bad).to(dev)] == -1).all() and ref["C"] > 1


# ---- (5) compaction ----

def _filter_and_compare(pkg, m, c, ref, keep):
    out = pkg.mesh.filter_components(m, c, keep)
    mv, mf, mn, mc = (a.cpu().numpy() for a in m)
    rv, rf, rn, rc = R.compact(mv, mf, ref["vert_comp"], ref["face_comp"], keep.cpu().numpy(), mn, mc)
    assert out.faces.dtype == torch.int32
    for got, want in zip(out, (rv, rf, rn, rc)):
        assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    return out


def test_compaction(pkg, dev):
    m, ref = _blob_mesh(pkg, dev)
    c = pkg.mesh.components(m.faces, len(m.verts), m.verts)
    sel = pkg.mesh.select_components
    out = pkg.mesh.filter_components(m, c, sel(c, min_faces=0))  # keep all: the input, bit for bit
    for a, b in zip(out, m):
        assert torch.equal(a, b)
    out = pkg.mesh.filter_components(m, c, torch.zeros(4, dtype=torch.bool, device=dev))  # keep none: the empty mesh
    assert [tuple(a.shape) for a in out] == [(0, 3)] * 4
    island_faces = int(c.n_faces.min())
    keep = sel(c, min_faces=island_faces + 1)
    assert keep.tolist() == R.select(ref["n_faces"], island_faces + 1).tolist() and int(keep.sum()) == 3
    out = _filter_and_compare(pkg, m, c, ref, keep)
    assert len(out.faces) == len(m.faces) - island_faces and int(out.faces.max()) == len(out.verts) - 1
    keep = sel(c, keep_largest=2)
    assert keep.tolist() == R.select(ref["n_faces"], 1, 2).tolist() and int(keep.sum()) == 2
    out = _filter_and_compare(pkg, m, c, ref, keep)
    again = pkg.mesh.components(out.faces, len(out.verts), out.verts)  # what is left are the two largest blobs
    assert sorted(again.n_faces.tolist()) == sorted(ref["n_faces"].tolist())[-2:]
    plain = pkg.mesh.filter_components(pkg.mesh.Mesh(m.verts, m.faces, None, None), c, keep)  # without normals and rgb
    assert plain.normals is None and plain.rgb is None and torch.equal(plain.verts, out.verts) and torch.equal(plain.faces, out.faces)


# the compaction's scan at the edges of its partition: a workgroup's CC_PTS = 2048 items (one total, exactly one, two), and the first V
# at which the scan of the totals gives a thread a run of two (more than 1024 totals).  Synthetic labels: no labelling runs.
@pytest.mark.parametrize("V,F", [(2047, 4100), (2048, 2048), (2049, 2049), (1024 * 2048, 5000), (1024 * 2048 + 1, 4097)])
def test_compaction_across_the_scan_partition(pkg, dev, V, F):
    rng = np.random.default_rng(V)
    vert_comp = (np.arange(V) % 3).astype(np.int32)
    face_comp = rng.integers(0, 3, F).astype(np.int32)
    faces = (3 * rng.integers(0, (V - 3) // 3 + 1, (F, 3)) + face_comp[:, None]).astype(np.int32)  # three vertices of the face's component
    assert faces.max() < V and np.array_equal(vert_comp[faces], np.repeat(face_comp[:, None], 3, 1))
    verts, normals, rgb = (rng.random((V, 3), dtype=np.float32) for _ in range(3))
    keep = np.array([1, 0, 1], np.uint8)
    rv, rf, rn, rc = R.compact(verts, faces, vert_comp, face_comp, keep, normals, rgb)
    assert len(rv) == V - (V + 1) // 3 and 0 < len(rf) < F
    t = lambda a: torch.from_numpy(a).to(dev)
    ov, of, on, oc, counts = pkg.ops.mesh_compact(t(verts), t(faces), t(normals), t(rgb), t(vert_comp), t(face_comp), t(keep), len(rv), len(rf))
    assert counts.tolist() == [len(rv), len(rf)]
    assert np.array_equal(of.cpu().numpy(), rf)
    for got, want in ((ov, rv), (on, rn), (oc, rc)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))


def test_compaction_stays_inside_its_capacities(pkg, dev):
    m, ref = _blob_mesh(pkg, dev)
    c = pkg.mesh.components(m.faces, len(m.verts), m.verts)
    keep = pkg.mesh.select_components(c, keep_largest=3)
    full = pkg.mesh.filter_components(m, c, keep)
    V1, F1 = len(full.verts), len(full.faces)
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F = len(m.verts), len(m.faces)
    ws = torch.empty(pkg._abi.mesh_cc_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    k8 = keep.to(torch.uint8)
    GUARD = 4096
    for cap_v, cap_f in ((V1 // 2, F1 // 3), (0, F1 // 2), (V1, 0), (V1 - 1, F1 - 1)):
        ov = torch.full((cap_v + GUARD, 3), 7.25, device=dev)
        on = torch.full((cap_v + GUARD, 3), -3.5, device=dev)
        oc = torch.full((cap_v + GUARD, 3), 1.5, device=dev)
        of = torch.full((cap_f + GUARD, 3), -77, dtype=torch.int32, device=dev)
        counts = torch.full((2,), -5, dtype=torch.int64, device=dev)
        pkg._abi.check(L.nerf_hip_mesh_cc_compact(m.verts.data_ptr(), m.normals.data_ptr(), m.rgb.data_ptr(), m.faces.data_ptr(), V, F,
                                                  c.vert_comp.data_ptr(), c.face_comp.data_ptr(), k8.data_ptr(), 4, ws.data_ptr(), ws.numel(),
                                                  ov.data_ptr(), on.data_ptr(), oc.data_ptr(), of.data_ptr(), cap_v, cap_f,
                                                  counts.data_ptr(), st))
        torch.cuda.synchronize()
        assert counts.tolist() == [V1, F1]
        assert (ov[cap_v:] == 7.25).all() and (on[cap_v:] == -3.5).all() and (oc[cap_v:] == 1.5).all() and (of[cap_f:] == -77).all()
        assert torch.equal(ov[:cap_v], full.verts[:cap_v]) and torch.equal(on[:cap_v], full.normals[:cap_v])
        assert torch.equal(oc[:cap_v], full.rgb[:cap_v]) and torch.equal(of[:cap_f], full.faces[:cap_f])


def test_stats_stay_inside_their_capacity(pkg, dev):
    v, f, ref = _random_mesh(0.9)
    c = pkg.mesh.components(torch.from_numpy(f).to(dev), len(v), torch.from_numpy(v).to(dev))
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    cap, GUARD = ref["C"] // 3, 1024
    nv = torch.full((cap + GUARD,), -9, dtype=torch.int32, device=dev)
    nf = torch.full((cap + GUARD,), -9, dtype=torch.int32, device=dev)
    lo = torch.full((cap + GUARD, 3), 2.5, device=dev)
    hi = torch.full((cap + GUARD, 3), 2.5, device=dev)
    vt = torch.from_numpy(v).to(dev)
    pkg._abi.check(L.nerf_hip_mesh_cc_stats(vt.data_ptr(), c.vert_comp.data_ptr(), c.face_comp.data_ptr(), len(v), len(f), nv.data_ptr(),
                                            nf.data_ptr(), lo.data_ptr(), hi.data_ptr(), cap, st))
    torch.cuda.synchronize()
    assert (nv[cap:] == -9).all() and (nf[cap:] == -9).all() and (lo[cap:] == 2.5).all() and (hi[cap:] == 2.5).all()
    assert torch.equal(nv[:cap], c.n_verts[:cap]) and torch.equal(nf[:cap], c.n_faces[:cap])
    assert torch.equal(lo[:cap], c.bbox_lo[:cap]) and torch.equal(hi[:cap], c.bbox_hi[:cap])


def test_host_refusals_launch_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F = 64, 32
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    ws = torch.full((pkg._abi.mesh_cc_ws_bytes(V, F),), 0x5A, dtype=torch.uint8, device=dev)
    changed = torch.full((1,), -5, dtype=torch.int32, device=dev)

    def rc_round(v=V, f=F, r=0, nbytes=ws.numel(), w=ws.data_ptr()):
        return L.nerf_hip_mesh_cc_round(faces.data_ptr(), v, f, r, w, nbytes, changed.data_ptr(), st)

    assert rc_round(v=-1) == -1 and rc_round(f=1 << 31) == -1 and rc_round(r=-1) == -1
    assert rc_round(nbytes=ws.numel() - 256) == -2 and rc_round(w=ws.data_ptr() + 4) == -1 and rc_round(w=None) == -1
    # the round past the cap: an error code of its own, a message that says so, nothing enqueued -- a caller's loop cannot hang
    assert rc_round(r=64) == -5
    with pytest.raises(pkg._abi.NerfHipError, match="did not converge"):
        pkg._abi.check(rc_round(r=64))
    with pytest.raises(pkg._abi.NerfHipError):
        pkg._abi.mesh_cc_ws_bytes(1 << 31, 0)
    torch.cuda.synchronize()
    assert int(changed) == -5 and (ws == 0x5A).all()
    with pytest.raises(ValueError):
        pkg.mesh.components(faces.to(torch.int64), V)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.components(faces.cpu(), V)


# ---- (7) filtering inside extract_mesh ----

@pytest.mark.parametrize("band", [None, 4])
def test_extract_mesh_filters_before_the_queries(oracle, pkg, dev, band):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    m = m.to(dev)
    lo, hi, shape = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), (37, 20, 45)
    level = float(m.density_grid(lo, hi, shape).median())
    kw = dict(normals="field", color=True, band=band)
    full = m.extract_mesh(lo, hi, shape, level, **kw)
    same = m.extract_mesh(lo, hi, shape, level, min_faces=None, keep_largest=None, **kw)
    for a, b in zip(full, same):
        assert torch.equal(a, b)
    c = pkg.mesh.components(full.faces, len(full.verts), full.verts)
    sizes = sorted(c.n_faces.tolist())
    print(f"band={band}: V={len(full.verts)} F={len(full.faces)} C={len(sizes)} largest {sizes[-3:]}")
    n = sizes[-1]  # keeps the largest component (and what ties with it)
    want = pkg.mesh.filter_components(full, c, pkg.mesh.select_components(c, min_faces=n))
    got = m.extract_mesh(lo, hi, shape, level, min_faces=n, **kw)
    assert len(got.faces) >= n > 0
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    want = pkg.mesh.filter_components(full, c, pkg.mesh.select_components(c, min_faces=2, keep_largest=2))
    got = m.extract_mesh(lo, hi, shape, level, min_faces=2, keep_largest=2, **kw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    grid = m.extract_mesh(lo, hi, shape, level, normals="grid", color=False, band=band, keep_largest=1)  # grid normals ride along
    unf = m.extract_mesh(lo, hi, shape, level, normals="grid", color=False, band=band)
    want = pkg.mesh.filter_components(unf, c, pkg.mesh.select_components(c, keep_largest=1))
    assert grid.rgb is None and all(torch.equal(a, b) for a, b in zip(grid[:3], want[:3]))
