"""GPU: edge topology, Taubin smoothing steps and face-derived vertex normals on the device (nerf_hip_mesh_edges_*,
nerf_hip_mesh_smooth_step, nerf_hip_mesh_vertex_normals; mesh.topology / mesh.smooth / mesh.vertex_normals; extract_mesh(smooth=))
against the numpy restatement in tests/smooth_reference.py.  Everything is exact equality: positions and normals as bits, degrees,
flags, counts and info."""
import numpy as np
import pytest
import torch

import simplify_meshes as M
import smooth_reference as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.int32)


def _mesh(pkg, dev, v, f):
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a copy: the inputs are read-only)
    return pkg.mesh.Mesh(t(np.asarray(v, dtype=np.float32)), t(np.asarray(f, dtype=np.int32)), None, None)


MESHES = {
    "blobs": lambda: M.blobs()[:2],
    "random": lambda: M.random_mesh()[:2],
    "fan": lambda: M.fan()[:2],
    "bad_input": lambda: M.bad_input()[:2],
    "patchwork": R.patchwork,
    "hub": R.hub,
    "book": R.book,
}
COUNT_KEYS = ("faces", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "used_verts", "max_degree")


def _want_counts(t):
    c = t["counts"]
    return dict(zip(COUNT_KEYS, c[:6] + c[7:]))


# ---- (1) topology ----

@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "patchwork", "book"])
def test_topology(pkg, dev, name):
    v, f = MESHES[name]()
    ref = R.topology(f, len(v))
    got = pkg.mesh.topology(torch.from_numpy(np.array(f)).to(dev), len(v))
    assert got.degree.dtype == torch.int32 and got.vert_flags.dtype == torch.int32 and got.degree.device.type == "cuda"
    assert np.array_equal(got.degree.cpu().numpy(), ref["degree"]) and np.array_equal(got.vert_flags.cpu().numpy(), ref["vert_flags"])
    assert {k: getattr(got, k) for k in COUNT_KEYS} == _want_counts(ref)
    assert got.euler == ref["euler"] and got.closed is ref["closed"]
    print(f"{name}: {got.summary()}")
    if name == "blobs":
        assert len(f) > 2048 and got.closed and got.euler == 8 and got.edges == 3078
    if name == "random":
        assert (got.edges, got.boundary_edges, got.max_degree) == (17583, 3738, 14)
    if name == "fan":  # 3000 faces on 300 vertices: shared keys in both orientations, from more than one workgroup of faces
        assert got.nonmanifold_edges > 50 and got.inconsistent_edges > 100 and (ref["tally"] < 0).any() and (ref["tally"] > 0).any()
    if name == "book":  # one key takes 3000 inserts, half in each direction
        assert ref["count"].max() == 3000 == len(f) and ref["tally"][ref["count"].argmax()] == 0 and got.max_degree == 3001
        assert (got.nonmanifold_edges, got.boundary_edges, got.inconsistent_edges) == (1, 6000, 0)
    if name == "bad_input":
        assert got.faces == len(f) - 60


# ---- (2) steps, with the normals of the result ----

def _check_smooth(pkg, dev, v, f, **kw):
    ref = R.smooth(v, f, **kw)
    m = _mesh(pkg, dev, v, f)
    out, info = pkg.mesh.smooth(m, **kw)
    assert out.faces is m.faces and out.rgb is None and out.verts.dtype == torch.float32 and tuple(out.verts.shape) == (len(v), 3)
    assert np.array_equal(_bits(out.verts), _bits(ref["verts"]))
    assert np.array_equal(_bits(out.normals), _bits(ref["normals"]))
    assert {k: info[k] for k in COUNT_KEYS} == _want_counts(ref["topo"])
    assert (info["pinned"], info["steps"], info["euler"], info["closed"]) == (ref["pinned"], ref["steps"], ref["topo"]["euler"], ref["topo"]["closed"])
    assert np.array_equal(info["lo"], ref["lo"]) and info["scale"] == ref["scale"]
    assert np.array_equal(_bits(m.verts), _bits(v)) and np.array_equal(m.faces.cpu().numpy(), f)  # the inputs are unchanged
    return out, info, ref


SMALL_BOX = {"blobs": ((8.0, 4.0, 9.0), 4.0), "random": ((5.0, 6.0, 4.0), 2.0), "fan": ((1.0, 0.3, 0.2), 0.25),
             "bad_input": ((5.0, 6.0, 4.0), 2.0), "patchwork": ((1.5, 0.25, 0.0), 1.0)}


@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "patchwork"])
def test_steps(pkg, dev, name):
    v, f = MESHES[name]()
    _, _, one = _check_smooth(pkg, dev, v, f, iterations=1)
    assert one["steps"] == 2
    _, _, three = _check_smooth(pkg, dev, v, f, iterations=3)
    if one["pinned"] < one["topo"]["counts"][5]:  # (the fan's vertices are all on boundary edges: pinned, nothing moves)
        assert not np.array_equal(_bits(three["verts"]), _bits(one["verts"]))
    _, _, free = _check_smooth(pkg, dev, v, f, iterations=3, fix_boundary=False)
    if one["pinned"]:
        assert free["pinned"] == 0 and not np.array_equal(_bits(free["verts"]), _bits(three["verts"]))
    _, _, lap = _check_smooth(pkg, dev, v, f, iterations=3, mu=None, lam=0.625)
    assert lap["steps"] == 3
    lo, scale = SMALL_BOX[name]
    uc, fin = R.box_coords(v, lo, scale)
    assert (uc[fin] == 2.0).any() and (uc[fin] == -1.0).any()  # vertices clamp on both sides of this box
    _check_smooth(pkg, dev, v, f, iterations=2, lo=lo, scale=scale)
    _, _, zero = _check_smooth(pkg, dev, v, f, iterations=0)
    assert zero["steps"] == 0 and np.array_equal(_bits(zero["verts"]), _bits(v))


def test_bad_vertices_are_skipped_and_copied(pkg, dev):
    v, f = MESHES["bad_input"]()
    bad = ~np.isfinite(v).all(1)
    far = np.abs(np.where(np.isfinite(v), v, 0)).max(1) > 1e29
    assert bad.sum() == 40 and far.sum() == 10
    out, _, ref = _check_smooth(pkg, dev, v, f, iterations=2, lo=(0.0, 0.0, 0.0), scale=16.0)
    assert np.array_equal(_bits(out.verts)[bad], _bits(v)[bad])  # NaN / +-inf rows keep their bits
    nbr_of_bad = np.zeros(len(v), bool)
    t = ref["topo"]
    nbr_of_bad[t["ea"][bad[t["eb"]]]] = True
    nbr_of_bad[t["eb"][bad[t["ea"]]]] = True
    assert nbr_of_bad.sum() > 20 and np.isfinite(out.verts.cpu().numpy()[~bad]).all()  # their neighbours moved on the finite ones alone


# ---- (3) normals ----

@pytest.mark.parametrize("name", ["blobs", "random", "fan", "bad_input", "patchwork", "hub", "book"])
def test_normals(pkg, dev, name):
    v, f = MESHES[name]()
    m = _mesh(pkg, dev, v, f)
    boxes = [(None, None)] + ([SMALL_BOX[name]] if name in SMALL_BOX else [])
    for lo, scale in boxes:
        got = pkg.mesh.vertex_normals(m.verts, m.faces, lo, scale)
        assert np.array_equal(_bits(got), _bits(R.vertex_normals(v, f, lo, scale)))
    assert np.array_equal(_bits(m.verts), _bits(v))
    if name == "blobs":
        got, mc = pkg.mesh.vertex_normals(m.verts, m.faces).cpu().numpy().astype(np.float64), M.blobs()[2].astype(np.float64)
        both = (np.abs(got).sum(1) > 0) & (np.abs(mc).sum(1) > 0)
        assert both.sum() > 1000 and ((got * mc).sum(1)[both] > 0).all()


# ---- (4) a hub: a row longer than a workgroup, one address taking 10 000 degree atomics ----

def test_book_steps(pkg, dev):
    v, f = R.book()
    for fix in (True, False):  # pinned: every vertex is on a boundary edge, nothing moves
        out, info, _ = _check_smooth(pkg, dev, v, f, iterations=2, fix_boundary=fix)
        assert info["pinned"] == (len(v) if fix else 0)


def test_hub(pkg, dev):
    v, f = R.hub()
    n = len(f)
    assert n == 5000 and len(v) == n + 1
    got = pkg.mesh.topology(torch.from_numpy(f.copy()).to(dev), len(v))
    assert got.max_degree == n and int(got.degree[n]) == n and got.edges == 2 * n and got.boundary_edges == n and not got.closed
    assert got.euler == 1  # a disc
    for fix in (True, False):
        out, info, ref = _check_smooth(pkg, dev, v, f, iterations=2, fix_boundary=fix)
        assert info["pinned"] == (n if fix else 0)
        assert not np.array_equal(_bits(out.verts)[n], _bits(v)[n])  # the hub moved, to the restatement's bits
    nrm = pkg.mesh.vertex_normals(*_mesh(pkg, dev, v, f)[:2])
    assert float(nrm[n, 2]) > 0.9


# ---- (5) sizes that cross the internal partitions ----

def test_empty_and_tiny_meshes(pkg, dev):
    e3 = np.zeros((0, 3), np.float32)
    ef = np.zeros((0, 3), np.int32)
    out, info, _ = _check_smooth(pkg, dev, e3, ef, iterations=2)
    assert info["edges"] == 0 and not info["closed"] and tuple(out.normals.shape) == (0, 3)
    v = M.random_mesh()[0]
    out, info, _ = _check_smooth(pkg, dev, v, ef, iterations=2)  # vertices without faces: nothing moves, no normal
    assert info["used_verts"] == 0 and np.array_equal(_bits(out.verts), _bits(v)) and not out.normals.any()
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    out, info, _ = _check_smooth(pkg, dev, tri, np.array([[0, 1, 2]], np.int32), iterations=1, fix_boundary=False)
    assert (info["edges"], info["boundary_edges"], info["euler"]) == (3, 3, 1)
    assert (out.normals.cpu().numpy() == [0, 0, 1]).all()
    t = pkg.mesh.topology(torch.from_numpy(ef).to(dev), 0)
    assert (t.faces, t.edges, t.euler, t.closed) == (0, 0, 0, False)
    assert len(M.blobs()[1]) == 2052 and len(M.random_mesh()[0]) == 5785  # (test_topology / test_steps: just over one scan block; odd)


# ---- (6) determinism ----

def test_two_runs_give_identical_bytes(pkg, dev):
    v, f = MESHES["random"]()
    m = _mesh(pkg, dev, v, f)
    a, ia = pkg.mesh.smooth(m, 3)
    b, ib = pkg.mesh.smooth(m, 3)
    assert torch.equal(a.verts.view(torch.int32), b.verts.view(torch.int32))
    assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    assert {k: ia[k] for k in ia if k != "lo"} == {k: ib[k] for k in ib if k != "lo"}
    c, _ = pkg.mesh.smooth(m, 3, normals=False)  # without the normal pass: the same positions, no normals
    assert c.normals is None and torch.equal(c.verts.view(torch.int32), a.verts.view(torch.int32))
    ta, tb = pkg.mesh.topology(m.faces, len(v)), pkg.mesh.topology(m.faces, len(v))
    assert torch.equal(ta.degree, tb.degree) and torch.equal(ta.vert_flags, tb.vert_flags) and ta[2:] == tb[2:]


# ---- (7) guard regions around every output and the workspace ----

def _raw(pkg, dev, v, f, lo, scale, cap_v, guard=4096):
    """the three C calls on guarded buffers -> (counts, degree, flags, step output, normals), each with `guard` rows behind it"""
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    m = _mesh(pkg, dev, v, f)
    V, F = len(v), len(f)
    nws = pkg._abi.mesh_edges_ws_bytes(V, F)
    ws = torch.full((nws + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((8 + 8,), -5, dtype=torch.int64, device=dev)
    degree = torch.full((V + guard,), -9, dtype=torch.int32, device=dev)
    flags = torch.full((V + guard,), -11, dtype=torch.int32, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_edges_build(m.faces.data_ptr(), V, F, ws.data_ptr(), nws, degree.data_ptr(), flags.data_ptr(),
                                               counts.data_ptr(), st))
    lo3 = pkg._abi.f32_array(lo)
    out = torch.full((cap_v + guard, 3), 7.25, device=dev)
    nrm = torch.full((cap_v + guard, 3), -3.5, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_smooth_step(m.verts.data_ptr(), out.data_ptr(), V, F, lo3, float(scale), 0.5, flags.data_ptr(),
                                               ws.data_ptr(), nws, cap_v, st))
    pkg._abi.check(L.nerf_hip_mesh_vertex_normals(m.verts.data_ptr(), m.faces.data_ptr(), V, F, lo3, float(scale), ws.data_ptr(), nws,
                                                  nrm.data_ptr(), cap_v, st))
    torch.cuda.synchronize()
    assert (ws[nws:] == 0x5A).all() and (counts[8:] == -5).all() and (degree[V:] == -9).all() and (flags[V:] == -11).all()
    assert np.array_equal(_bits(m.verts), _bits(v)) and np.array_equal(m.faces.cpu().numpy(), f)
    return counts[:8].tolist(), degree[:V], flags[:V], out, nrm


def test_outputs_stay_inside_their_capacities(pkg, dev):
    v, f = MESHES["bad_input"]()
    lo, scale = (0.0, 0.0, 0.0), 16.0
    t = R.topology(f, len(v))
    want_v = R.step(v, t, lo, scale, 0.5)
    want_n = R.vertex_normals(v, f, lo, scale)
    V = len(v)
    for cap_v in (V, V // 2, 0, V - 1, V + 100):
        counts, degree, flags, out, nrm = _raw(pkg, dev, v, f, lo, scale, cap_v)
        k = min(cap_v, V)
        assert counts == t["counts"]
        assert np.array_equal(degree.cpu().numpy(), t["degree"]) and np.array_equal(flags.cpu().numpy(), t["vert_flags"])
        assert (out[k:] == 7.25).all() and (nrm[k:] == -3.5).all()
        assert np.array_equal(_bits(out[:k]), _bits(want_v[:k])) and np.array_equal(_bits(nrm[:k]), _bits(want_n[:k]))


# ---- (8) refusals on the host: nothing is launched ----

def test_host_refusals_launch_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F = 64, 32
    verts = torch.zeros(V, 3, device=dev)
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    need = pkg._abi.mesh_edges_ws_bytes(V, F)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((8,), -5, dtype=torch.int64, device=dev)
    degree = torch.full((V,), -9, dtype=torch.int32, device=dev)
    flags = torch.full((V,), -11, dtype=torch.int32, device=dev)
    out = torch.full((V, 3), 2.5, device=dev)

    def build(v=V, f=F, w=ws.data_ptr(), nbytes=need, fp=faces.data_ptr(), dp=degree.data_ptr(), cp=counts.data_ptr()):
        return L.nerf_hip_mesh_edges_build(fp, v, f, w, nbytes, dp, flags.data_ptr(), cp, st)

    def step(v=V, f=F, lo=(0, 0, 0), scale=1.0, wt=0.5, w=ws.data_ptr(), nbytes=need, ip=verts.data_ptr(), op=out.data_ptr(), cap=V):
        return L.nerf_hip_mesh_smooth_step(ip, op, v, f, pkg._abi.f32_array(lo), scale, wt, None, w, nbytes, cap, st)

    def normals(v=V, f=F, lo=(0, 0, 0), scale=1.0, w=ws.data_ptr(), nbytes=need, vp=verts.data_ptr(), op=out.data_ptr(), cap=V):
        return L.nerf_hip_mesh_vertex_normals(vp, faces.data_ptr(), v, f, pkg._abi.f32_array(lo), scale, w, nbytes, op, cap, st)

    nan, inf = float("nan"), float("inf")
    for call in (build, step, normals):
        assert call(v=-1) == -1 and call(f=1 << 31) == -1 and call(w=None) == -1 and call(w=ws.data_ptr() + 4) == -1
        assert call(nbytes=need - 1) == -2  # one byte short
    assert build(fp=None) == -1 and build(dp=None) == -1 and build(cp=None) == -1 and build(cp=counts.data_ptr() + 4) == -1
    for call in (step, normals):
        for scale in (0.0, -1.0, nan, inf):
            assert call(scale=scale) == -1
        assert call(lo=(0, nan, 0)) == -1 and call(lo=(inf, 0, 0)) == -1 and call(cap=-1) == -1 and call(op=None) == -1
    assert step(wt=nan) == -1 and step(wt=inf) == -1 and step(ip=None) == -1 and normals(vp=None) == -1
    assert step(op=verts.data_ptr()) == -1 and step(op=verts.data_ptr() + 12 * (V - 1)) == -1  # the output overlaps the input
    with pytest.raises(pkg._abi.NerfHipError):
        pkg._abi.mesh_edges_ws_bytes(-1, 0)
    torch.cuda.synchronize()
    assert (counts == -5).all() and (ws == 0x5A).all() and (out == 2.5).all() and (degree == -9).all() and (flags == -11).all()
    m = pkg.mesh.Mesh(verts, faces, None, None)
    for kw in (dict(lam=nan), dict(mu=inf), dict(scale=nan), dict(scale=0.0), dict(scale=-2.0), dict(iterations=-1), dict(lo=(0, nan, 0))):
        with pytest.raises(ValueError):
            pkg.mesh.smooth(m, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.smooth(pkg.mesh.Mesh(verts.cpu(), faces.cpu(), None, None))
    torch.cuda.synchronize()
    assert (counts == -5).all() and (ws == 0x5A).all() and (out == 2.5).all()
    assert build() == 0 and step() == 0 and normals() == 0  # and the good calls go through
    torch.cuda.synchronize()
    assert counts.tolist() == [0] * 8 and (degree == 0).all() and (out == 0).all()  # every face repeats index 0: none takes part


# ---- (9) inside extract_mesh ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


LO, HI, RES = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), 24


@pytest.mark.parametrize("min_faces,simplify", [(None, None), (8, 2)])
def test_extract_mesh_smooths_between_filter_and_simplify(pkg, dev, model, min_faces, simplify):
    from nerf_tiny_amd.nerf import field_normals, grid_step, simplify_lattice_of_grid, smooth_scale_of_grid

    m = model
    level = float(m.density_grid(LO, HI, RES).median())
    kw = dict(min_faces=min_faces)
    base = m.extract_mesh(LO, HI, RES, level, normals="grid", color=False, **kw)  # the earlier stages' mesh
    same = m.extract_mesh(LO, HI, RES, level, normals="grid", color=False, smooth=None, **kw)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base[:3], same[:3]))
    lo32, hi32 = np.asarray(LO, np.float32), np.asarray(HI, np.float32)
    scale = smooth_scale_of_grid(lo32, hi32)
    assert scale == np.float32(4.0)  # the box is 2.4 x 1.25 x 2.45
    want, info = pkg.mesh.smooth(pkg.mesh.Mesh(base.verts, base.faces, None, None), 2, lo=lo32, scale=scale)
    assert info["steps"] == 4 and info["edges"] > 100 and not torch.equal(want.verts, base.verts)
    if simplify is not None:
        cell, dims = simplify_lattice_of_grid(grid_step(lo32, hi32, (RES,) * 3), (RES,) * 3, simplify)
        want_field, _ = pkg.mesh.simplify(pkg.mesh.Mesh(want.verts, want.faces, None, None), cell, lo32, dims)
        want, _ = pkg.mesh.simplify(want, cell, lo32, dims)
        assert torch.equal(want_field.verts, want.verts)
    kw.update(simplify=simplify, smooth=2)
    got = m.extract_mesh(LO, HI, RES, level, normals="grid", color=True, **kw)
    assert torch.equal(got.verts.view(torch.int32), want.verts.view(torch.int32)) and torch.equal(got.faces, want.faces)
    assert torch.equal(got.normals.view(torch.int32), want.normals.view(torch.int32))
    assert torch.equal(got.rgb, m.query(got.verts, -got.normals)[0])
    fld = m.extract_mesh(LO, HI, RES, level, normals="field", color=True, **kw)
    assert torch.equal(fld.verts.view(torch.int32), want.verts.view(torch.int32)) and torch.equal(fld.faces, want.faces)
    nrm = field_normals(m.query_grad(fld.verts)[2])
    assert torch.equal(fld.normals, nrm) and torch.equal(fld.rgb, m.query(fld.verts, -nrm)[0])
    print(f"min_faces={min_faces} simplify={simplify}: V {len(base.verts)} -> {len(got.verts)}, {info}")
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            m.extract_mesh(LO, HI, RES, level, smooth=bad)
