"""CPU: the vectorised restatement of the vertex-clustering simplification (tests/simplify_reference.py) against a plain-loop reading
of the definition in include/nerf_hip.h, and the invariants of its output, on the meshes the GPU tests use."""
import numpy as np
import pytest

import simplify_meshes as M
import simplify_reference as R


def _case(name):
    if name.startswith("blobs"):
        v, f, n = M.blobs()
        return v, f, n, M.grid_lattice(24, int(name[5:]))
    v, f, n = M.random_mesh()
    if name == "random3":
        return v, f, n, M.grid_lattice(16, 3)
    lo, cell, dims = R.default_lattice(v, M.ANISO["cell"], M.ANISO["lo"])
    return v, f, n, (lo, cell, dims)


CASES = ["blobs2", "blobs3", "blobs5", "random3", "aniso"]


@pytest.mark.parametrize("name", CASES)
def test_vectorised_equals_loops(name):
    v, f, n, (lo, cell, dims) = _case(name)
    r = R.simplify(v, f, n, lo, cell, dims)
    lv, lf, ln, lc, ldeg, ldup = R.simplify_loops(v, f, n, lo, cell, dims)
    assert np.array_equal(r["verts"].view(np.int32), lv.view(np.int32))
    assert np.array_equal(r["normals"].view(np.int32), ln.view(np.int32))
    assert np.array_equal(r["faces"], lf) and r["faces"].dtype == np.int32
    assert (r["clusters"], r["degenerate_faces"], r["duplicate_faces"]) == (lc, ldeg, ldup)
    plain = R.simplify(v, f, None, lo, cell, dims)
    assert plain["normals"] is None and np.array_equal(plain["verts"], r["verts"]) and np.array_equal(plain["faces"], r["faces"])
    print(f"{name}: V {len(v)} -> {len(lv)}, F {len(f)} -> {len(lf)}, clusters {lc}, degenerate {ldeg}, duplicates {ldup}, "
          f"unreferenced {r['unreferenced']}, opposite pairs {r['opposite_pairs']}")


def test_the_inputs_still_bite():
    """every rule of the definition is exercised: same-orientation duplicates, opposite pairs, unreferenced clusters, the island"""
    v, f, n = M.blobs()
    b3 = R.simplify(v, f, n, *M.grid_lattice(24, 3))
    assert b3["unreferenced"] >= 1  # the one-cell island collapses away (and a cap of a ball)
    assert 0 < len(b3["faces"]) < len(f) // 4 and b3["degenerate_faces"] > len(f) // 2
    isl = np.asarray(M.ISLAND) // 3
    assert (isl[0] * 8 + isl[1]) * 8 + isl[2] not in b3["cells"].tolist()
    v, f, n = M.random_mesh()
    r3 = R.simplify(v, f, n, *M.grid_lattice(16, 3))
    assert r3["duplicate_faces"] >= 1 and r3["opposite_pairs"] >= 1
    an = R.simplify(v, f, n, *R.default_lattice(v, M.ANISO["cell"], M.ANISO["lo"]))
    assert an["duplicate_faces"] >= 1 and an["opposite_pairs"] >= 1
    # vertices below the given lo are pulled to the lattice's face
    assert (v[:, 1] >= 0).all() and (v[:, 0] < 0.25).any()


@pytest.mark.parametrize("name", CASES)
def test_invariants(name):
    v, f, n, (lo, cell, dims) = _case(name)
    lo, cell, dims = R.lattice(lo, cell, dims)
    r = R.simplify(v, f, n, lo, cell, dims)
    ov, of = r["verts"], r["faces"]
    assert ((of >= 0) & (of < len(ov))).all()
    assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
    k = np.argmin(of, axis=1)
    canon = np.take_along_axis(of, (k[:, None] + np.arange(3)) % 3, axis=1)
    assert len(np.unique(canon, axis=0)) == len(of)  # no two kept faces are equal up to rotation
    assert np.array_equal(np.unique(of), np.arange(len(ov)))  # every output vertex is referenced
    assert (np.diff(r["cells"]) > 0).all() and len(r["cells"]) == len(ov)  # ascending cell index
    assert (np.diff(r["kept"]) > 0).all()  # kept faces in input order
    # every output vertex inside its cell's closed box, up to one fp32 rounding of the box corners
    c = r["cells"]
    ijk = np.stack([c // (dims[1] * dims[2]), c // dims[2] % dims[1], c % dims[2]], 1).astype(np.float64)
    box_lo = (lo.astype(np.float64) + ijk * cell.astype(np.float64)).astype(np.float32)
    box_hi = (lo.astype(np.float64) + (ijk + 1) * cell.astype(np.float64)).astype(np.float32)
    assert (ov >= np.nextafter(box_lo, np.float32(-np.inf))).all() and (ov <= np.nextafter(box_hi, np.float32(np.inf))).all()
    nl = np.linalg.norm(r["normals"].astype(np.float64), axis=1)
    assert ((np.abs(nl - 1) < 1e-6) | (nl == 0)).all()  # unit, or (0, 0, 0) where the sum vanishes


def test_fan_and_bad_input():
    v, f, lo, cell, dims = M.fan()
    r = R.simplify(v, f, None, lo, cell, dims)
    assert r["kept"].tolist() == [0, 1] and len(r["verts"]) == 3 and r["duplicate_faces"] == 2998 and r["opposite_pairs"] == 1
    perm = np.random.default_rng(11).permutation(len(f))
    rp = R.simplify(v, f[perm], None, lo, cell, dims)
    assert len(rp["kept"]) == 2 and rp["kept"][0] == 0 and np.array_equal(rp["verts"], r["verts"])
    lv, lf, _, _, _, ldup = R.simplify_loops(v, f[perm], None, lo, cell, dims)
    assert np.array_equal(lf, rp["faces"]) and ldup == 2998
    bv, bf, bn, lo, cell, dims = M.bad_input()
    r = R.simplify(bv, bf, bn, lo, cell, dims)
    lv, lf, ln, lc, ldeg, ldup = R.simplify_loops(bv, bf, bn, lo, cell, dims)
    assert np.array_equal(r["verts"].view(np.int32), lv.view(np.int32)) and np.array_equal(r["normals"].view(np.int32), ln.view(np.int32))
    assert np.array_equal(r["faces"], lf) and (r["clusters"], r["degenerate_faces"], r["duplicate_faces"]) == (lc, ldeg, ldup)
    assert np.isfinite(r["verts"]).all() and np.isfinite(r["normals"]).all() and len(lf) > 50


def test_default_lattice():
    v, _, _ = M.random_mesh()
    lo, cell, dims = R.default_lattice(v, 3.0)
    assert np.array_equal(lo, v.min(0)) and dims.tolist() == [6, 6, 6]
    lin, _ = R.vertex_cells(v, lo, cell, dims)
    assert lin.min() >= 0 and lin.max() < 216
    w = v.copy()
    w[5] = np.nan
    w[7, 1] = np.inf
    assert np.array_equal(R.default_lattice(w, 3.0)[2], dims)
    assert R.default_lattice(np.full((4, 3), np.nan, np.float32), 1.0)[2].tolist() == [1, 1, 1]
    assert R.default_lattice(v, 1e-6)[2].tolist() == [2048] * 3
