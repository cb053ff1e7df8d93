"""GPU: mesh simplification by vertex clustering on the device (nerf_hip_mesh_simplify_*, mesh.simplify, extract_mesh(simplify=))
against the numpy restatement in tests/simplify_reference.py.  Everything is exact equality: vertices and normals as bits, faces,
counts and info."""
import numpy as np
import pytest
import torch

import simplify_meshes as M
import simplify_reference as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.int32)


def _mesh(pkg, dev, v, f, n=None):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (a copy: the inputs are read-only)
    return pkg.mesh.Mesh(t(v), t(np.asarray(f, dtype=np.int32)), t(n), None)


def _check(pkg, dev, v, f, n, lo, cell, dims):
    """mesh.simplify of (v, f, n) over the lattice equals the restatement; -> (Mesh, info, reference dict)"""
    ref = R.simplify(v, f, n, lo, cell, dims)
    out, info = pkg.mesh.simplify(_mesh(pkg, dev, v, f, n), cell, lo, dims)
    assert out.verts.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.rgb is None and out.verts.device.type == "cuda"
    assert tuple(out.verts.shape) == ref["verts"].shape and tuple(out.faces.shape) == ref["faces"].shape
    assert np.array_equal(_bits(out.verts), _bits(ref["verts"]))
    assert np.array_equal(out.faces.cpu().numpy(), ref["faces"])
    if n is None:
        assert out.normals is None
    else:
        assert np.array_equal(_bits(out.normals), _bits(ref["normals"]))
    want = dict(verts_in=len(v), faces_in=len(f), verts_out=len(ref["verts"]), faces_out=len(ref["faces"]), clusters=ref["clusters"],
                degenerate_faces=ref["degenerate_faces"], duplicate_faces=ref["duplicate_faces"])
    assert {k: info[k] for k in want} == want
    return out, info, ref


# ---- (1) blobs, with normals ----

@pytest.mark.parametrize("k", [2, 3, 5])
def test_blobs(pkg, dev, k):
    v, f, n = M.blobs()
    out, info, ref = _check(pkg, dev, v, f, n, *M.grid_lattice(24, k))
    print(f"blobs k={k}: {info}")
    if k == 3:  # the island and the unreferenced clusters are gone
        assert info["clusters"] - info["verts_out"] == ref["unreferenced"] >= 1
        isl = np.asarray(M.ISLAND) // 3
        assert (isl[0] * 8 + isl[1]) * 8 + isl[2] not in ref["cells"].tolist()
        comps = pkg.mesh.components(out.faces, len(out.verts))
        assert len(comps.n_faces) == 3  # the three balls


# ---- (2) the random mesh: V and F no multiple of a wave or a workgroup; 8000 cells are more than one scan workgroup ----

@pytest.mark.parametrize("name", ["k2", "k3", "aniso", "k0.75"])
def test_random_field(pkg, dev, name):
    v, f, n = M.random_mesh()
    assert len(v) % 64 and len(f) % 64 and len(v) % 256 and len(f) % 256
    if name == "aniso":
        lat = R.default_lattice(v, M.ANISO["cell"], M.ANISO["lo"])
    elif name == "k0.75":
        lat = ((0.0, 0.0, 0.0), (np.float32(0.75),) * 3, (20, 20, 20))
        assert 20 ** 3 > 2048
    else:
        lat = M.grid_lattice(16, int(name[1:]))
    _, info, ref = _check(pkg, dev, v, f, n, *lat)
    print(f"random {name}: {info}")
    if name in ("k3", "aniso"):
        assert ref["duplicate_faces"] >= 1 and ref["opposite_pairs"] >= 1


def test_lattice_of_more_cells_than_one_scan_run(pkg, dev):
    """129 x 128 x 128 = 2,113,536 cells are more than 1024 workgroup totals of 2048: every thread of the totals' scan takes a run of
    two.  The corner at x = -1 puts the mesh's cells up to the lattice's last plane, so the last totals are not empty."""
    v, f, n = M.random_mesh()
    lo, cell, dims = (-1.0, 0.0, 0.0), (np.float32(0.125),) * 3, (129, 128, 128)
    assert dims[0] * dims[1] * dims[2] > 1024 * 2048 and max(dims) <= 2048
    _, info, ref = _check(pkg, dev, v, f, n, lo, cell, dims)
    assert ref["cells"].min() < 2048 * 128 and ref["cells"].max() >= 2048 * 1030  # occupied cells in the first and in the last runs
    assert info["faces_out"] > 1000


def test_default_lattice(pkg, dev):
    v, f, n = M.random_mesh()
    lo, cell, dims = R.default_lattice(v, 3.0)
    got = pkg.mesh.simplify_lattice(torch.from_numpy(v.copy()).to(dev), 3.0)
    assert np.array_equal(got[0], lo) and np.array_equal(got[1], cell) and np.array_equal(got[2], dims)
    out, info = pkg.mesh.simplify(_mesh(pkg, dev, v, f, n), 3.0)
    ref = R.simplify(v, f, n, lo, cell, dims)
    assert np.array_equal(_bits(out.verts), _bits(ref["verts"])) and np.array_equal(out.faces.cpu().numpy(), ref["faces"])
    assert info["dims"] == tuple(dims.tolist()) and np.array_equal(info["lo"], lo)
    lo2 = (-1.0, 0.5, 0.0)  # a given corner: the default dims cover the maximum from there
    out, info = pkg.mesh.simplify(_mesh(pkg, dev, v, f, n), (2.0, 3.0, 4.0), lo=lo2)
    ref = R.simplify(v, f, n, *R.default_lattice(v, (2.0, 3.0, 4.0), lo2))
    assert np.array_equal(_bits(out.verts), _bits(ref["verts"])) and np.array_equal(out.faces.cpu().numpy(), ref["faces"])


# ---- (3) one cell holds the whole mesh: every atomic goes to the same words ----

def test_one_cell(pkg, dev):
    v, f, n = M.random_mesh()
    out, info, _ = _check(pkg, dev, v, f, n, (0.0, 0.0, 0.0), (16.0, 16.0, 16.0), (1, 1, 1))
    assert info["verts_out"] == 0 and info["faces_out"] == 0 and info["clusters"] == 1 and info["degenerate_faces"] == len(f)
    assert tuple(out.verts.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.normals.shape) == (0, 3)


# ---- (4) the fan: 3000 faces over more than one workgroup share two keys ----

def test_fan(pkg, dev):
    v, f, lo, cell, dims = M.fan()
    assert len(f) > 2048
    out, info, ref = _check(pkg, dev, v, f, None, lo, cell, dims)
    assert ref["kept"].tolist() == [0, 1] and info["faces_out"] == 2 and info["verts_out"] == 3 and info["duplicate_faces"] == 2998
    cells = lambda face: (v[face, 0] // 1).astype(int).tolist()
    assert out.faces.cpu().numpy().tolist() == [cells(f[0]), cells(f[1])]  # the first face of each orientation, in its own corner order
    perm = np.random.default_rng(11).permutation(len(f))
    outp, _, refp = _check(pkg, dev, v, f[perm], None, lo, cell, dims)
    assert len(refp["kept"]) == 2 and refp["kept"][0] == 0
    assert outp.faces.cpu().numpy().tolist() == [cells(f[perm][j]) for j in refp["kept"]]
    assert torch.equal(outp.verts, out.verts)


# ---- (5) bad input ----

def test_bad_input(pkg, dev):
    v, f, n, lo, cell, dims = M.bad_input()
    _, info, ref = _check(pkg, dev, v, f, n, lo, cell, dims)
    assert info["faces_out"] > 50 and np.isfinite(ref["verts"]).all()
    print(f"bad input: {info}")


def _raw(pkg, dev, v, f, n, lo, cell, dims, cap_v, cap_f, guard=4096):
    """the two C calls on guarded buffers -> (counts, out_verts, out_normals, out_faces) with `guard` rows behind each capacity"""
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    m = _mesh(pkg, dev, v, f, n)
    V, F = len(v), len(f)
    lo3, cell3, dims3 = pkg._abi.f32_array(lo), pkg._abi.f32_array(cell), pkg._abi.i32_array(dims)
    nws = pkg._abi.mesh_simplify_ws_bytes(V, F, dims)
    ws = torch.full((nws + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((6 + 8,), -5, dtype=torch.int64, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_simplify_count(m.verts.data_ptr(), m.normals.data_ptr(), m.faces.data_ptr(), V, F, lo3, cell3, dims3,
                                                  ws.data_ptr(), nws, counts.data_ptr(), st))
    ov = torch.full((cap_v + guard, 3), 7.25, device=dev)
    on = torch.full((cap_v + guard, 3), -3.5, device=dev)
    of = torch.full((cap_f + guard, 3), -77, dtype=torch.int32, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_simplify_emit(m.faces.data_ptr(), V, F, lo3, cell3, dims3, ws.data_ptr(), nws, ov.data_ptr(), on.data_ptr(),
                                                 of.data_ptr(), cap_v, cap_f, st))
    torch.cuda.synchronize()
    assert (ws[nws:] == 0x5A).all() and (counts[6:] == -5).all()
    return counts[:6].tolist(), ov, on, of


def test_outputs_stay_inside_their_capacities(pkg, dev):
    v, f, n, lo, cell, dims = M.bad_input()
    ref = R.simplify(v, f, n, lo, cell, dims)
    V1, F1 = len(ref["verts"]), len(ref["faces"])
    for cap_v, cap_f in ((V1, F1), (V1 // 2, F1 // 3), (0, F1 // 2), (V1, 0), (V1 - 1, F1 - 1)):
        counts, ov, on, of = _raw(pkg, dev, v, f, n, lo, cell, dims, cap_v, cap_f)
        assert counts == [V1, F1, ref["clusters"], 0, ref["degenerate_faces"], ref["duplicate_faces"]]
        assert (ov[cap_v:] == 7.25).all() and (on[cap_v:] == -3.5).all() and (of[cap_f:] == -77).all()
        assert np.array_equal(_bits(ov[:cap_v]), _bits(ref["verts"][:cap_v])) and np.array_equal(_bits(on[:cap_v]), _bits(ref["normals"][:cap_v]))
        assert np.array_equal(of[:cap_f].cpu().numpy(), ref["faces"][:cap_f])


# ---- (6), (7) determinism; without normals ----

def test_two_runs_give_identical_bytes(pkg, dev):
    v, f, n = M.random_mesh()
    m = _mesh(pkg, dev, v, f, n)
    a, ia = pkg.mesh.simplify(m, 2.0, (0, 0, 0), (8, 8, 8))
    b, ib = pkg.mesh.simplify(m, 2.0, (0, 0, 0), (8, 8, 8))
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert {k: ia[k] for k in ia if k not in ("lo", "cell")} == {k: ib[k] for k in ib if k not in ("lo", "cell")}


def test_without_normals(pkg, dev):
    v, f, n = M.blobs()
    lat = M.grid_lattice(24, 2)
    with_n, _, _ = _check(pkg, dev, v, f, n, *lat)
    plain, _, _ = _check(pkg, dev, v, f, None, *lat)
    assert plain.normals is None and torch.equal(plain.verts, with_n.verts) and torch.equal(plain.faces, with_n.faces)


def test_empty_meshes(pkg, dev):
    out, info = pkg.mesh.simplify(_mesh(pkg, dev, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), 1.0)
    assert info["verts_out"] == 0 and info["faces_out"] == 0 and info["clusters"] == 0
    v = M.random_mesh()[0]
    out, info = pkg.mesh.simplify(_mesh(pkg, dev, v, np.zeros((0, 3), np.int32)), 2.0)  # vertices without faces: clusters, no output
    assert info["verts_out"] == 0 and info["clusters"] == R.simplify(v, np.zeros((0, 3), np.int32), None, *R.default_lattice(v, 2.0))["clusters"] > 0


# ---- (8) bad lattices are refused and enqueue nothing ----

def test_host_refusals_launch_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    V, F = 64, 32
    verts = torch.zeros(V, 3, device=dev)
    faces = torch.zeros(F, 3, dtype=torch.int32, device=dev)
    ws = torch.full((pkg._abi.mesh_simplify_ws_bytes(V, F, (4, 4, 4)),), 0x5A, dtype=torch.uint8, device=dev)
    counts = torch.full((6,), -5, dtype=torch.int64, device=dev)
    out = torch.full((V, 3), 2.5, device=dev)
    outf = torch.full((F, 3), -7, dtype=torch.int32, device=dev)

    def rc(lo=(0, 0, 0), cell=(1, 1, 1), dims=(4, 4, 4), v=V, f=F, nbytes=ws.numel(), w=ws.data_ptr()):
        a = (pkg._abi.f32_array(lo), pkg._abi.f32_array(cell), pkg._abi.i32_array(dims), w, nbytes)
        r1 = L.nerf_hip_mesh_simplify_count(verts.data_ptr(), None, faces.data_ptr(), v, f, *a, counts.data_ptr(), st)
        r2 = L.nerf_hip_mesh_simplify_emit(faces.data_ptr(), v, f, *a, out.data_ptr(), None, outf.data_ptr(), V, F, st)
        assert r1 == r2
        return r1

    nan, inf = float("nan"), float("inf")
    for cell in ((0, 1, 1), (1, -1, 1), (1, 1, nan), (inf, 1, 1)):
        assert rc(cell=cell) == -1
    for dims in ((0, 4, 4), (4, 2049, 4), (4, 4, -1), (2048, 2048, 512)):
        assert rc(dims=dims) == -1
    assert rc(lo=(0, nan, 0)) == -1 and rc(lo=(inf, 0, 0)) == -1
    assert rc(v=-1) == -1 and rc(f=1 << 31) == -1 and rc(w=None) == -1 and rc(w=ws.data_ptr() + 4) == -1
    assert rc(nbytes=ws.numel() - 256) == -2
    with pytest.raises(pkg._abi.NerfHipError, match="2048"):
        pkg._abi.mesh_simplify_ws_bytes(V, F, (4, 4096, 4))
    torch.cuda.synchronize()
    assert (counts == -5).all() and (ws == 0x5A).all() and (out == 2.5).all() and (outf == -7).all()
    m = pkg.mesh.Mesh(verts, faces, None, None)
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.mesh.simplify(m, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.simplify(pkg.mesh.Mesh(verts.cpu(), faces.cpu(), None, None), 1.0)
    assert rc() == 0  # and the good call goes through
    torch.cuda.synchronize()


# ---- (9) inside extract_mesh ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


LO, HI, RES = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), 24


@pytest.mark.parametrize("band,keep_largest", [(None, None), (4, 1)])
def test_extract_mesh_simplifies_before_the_queries(pkg, dev, model, band, keep_largest):
    from nerf_tiny_amd.nerf import field_normals, grid_step, simplify_lattice_of_grid

    m = model
    level = float(m.density_grid(LO, HI, RES).median())
    kw = dict(band=band, keep_largest=keep_largest)
    base = m.extract_mesh(LO, HI, RES, level, normals="grid", color=False, **kw)  # the unsimplified, filtered mesh
    same = m.extract_mesh(LO, HI, RES, level, normals="grid", color=False, simplify=None, **kw)
    assert all(torch.equal(a, b) for a, b in zip(base[:3], same[:3]))
    lo32 = np.asarray(LO, np.float32)
    step = grid_step(lo32, np.asarray(HI, np.float32), (RES,) * 3)
    for k in (2, 3):
        cell, dims = simplify_lattice_of_grid(step, (RES,) * 3, k)
        assert np.array_equal(cell, (np.float32(k) * step).astype(np.float32)) and dims == [-(-(RES - 1) // k)] * 3
        want, info = pkg.mesh.simplify(base, cell, lo32, dims)
        assert 0 < info["faces_out"] < len(base.faces) // 2
        got = m.extract_mesh(LO, HI, RES, level, normals="grid", color=True, simplify=k, **kw)
        assert torch.equal(got.verts, want.verts) and torch.equal(got.faces, want.faces)
        assert torch.equal(got.normals.view(torch.int32), want.normals.view(torch.int32))
        assert torch.equal(got.rgb, m.query(got.verts, -got.normals)[0])
        fld = m.extract_mesh(LO, HI, RES, level, normals="field", color=True, simplify=k, **kw)
        assert torch.equal(fld.verts, want.verts) and torch.equal(fld.faces, want.faces)
        nrm = field_normals(m.query_grad(fld.verts)[2])
        assert torch.equal(fld.normals, nrm) and torch.equal(fld.rgb, m.query(fld.verts, -nrm)[0])
        print(f"band={band} keep_largest={keep_largest} k={k}: V {len(base.verts)} -> {len(got.verts)}, F {len(base.faces)} -> {len(got.faces)}")
    with pytest.raises(ValueError):
        m.extract_mesh(LO, HI, RES, level, simplify=1)
