"""CPU: the numpy restatement of the mesh-component calls (tests/cc_reference.py) against a brute-force flood fill on hand-made
meshes; mesh.select_components; the command line.  The device kernels are held to the restatement in
tests/test_gpu_mesh_components.py."""
import importlib
import os

import numpy as np
import pytest
import torch

import cc_reference as R
from conftest import ROOT


def _flood(faces, V):
    """Components by repeated flood fill over an adjacency matrix: (vert_comp, face_comp, n_verts, n_faces), ids in the order in which a
    scan over the vertices first meets each component (= ascending smallest index)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = [all(0 <= i < V for i in t) for t in f.tolist()]
    adj = np.eye(V, dtype=bool)
    for t, good in zip(f.tolist(), ok):
        if good:
            for u in t:
                for w in t:
                    adj[u, w] = True
    comp = np.full(V, -1, np.int64)
    C = 0
    for v in range(V):
        if comp[v] >= 0:
            continue
        seen = np.zeros(V, bool)
        seen[v] = True
        while True:
            grown = adj[seen].any(axis=0) | seen
            if (grown == seen).all():
                break
            seen = grown
        comp[seen] = C
        C += 1
    face_comp = np.array([comp[t[0]] if good else -1 for t, good in zip(f.tolist(), ok)], dtype=np.int64).reshape(len(f))
    n_verts = np.array([(comp == c).sum() for c in range(C)], dtype=np.int64)
    n_faces = np.array([(face_comp == c).sum() for c in range(C)], dtype=np.int64)
    return comp, face_comp, n_verts, n_faces


BOW_TIE = ([[0, 1, 2], [2, 3, 4]], 5)  # two triangles that share one vertex: one component
CASES = {
    "bow_tie": BOW_TIE,
    "isolated_vertex": ([[0, 1, 2], [4, 5, 6]], 8),  # 3 and 7 are in no face
    "duplicate_and_degenerate": ([[5, 5, 2], [0, 1, 3], [0, 1, 3], [3, 1, 0], [4, 4, 4], [2, 6, 6]], 8),
    "out_of_range": ([[0, 1, 2], [2, 3, -1], [3, 4, 5], [5, 6, 7], [7, 8, 9], [0, 9, 10]], 10),
    "late_merge": ([[8, 9, 7], [0, 1, 2], [3, 4, 5], [5, 6, 7], [2, 9, 9]], 10),
    "no_faces": (np.zeros((0, 3), np.int64), 4),
    "no_vertices": (np.zeros((0, 3), np.int64), 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_a_flood_fill(name):
    faces, V = CASES[name]
    r = R.components(faces, V)
    comp, face_comp, n_verts, n_faces = _flood(faces, V)
    assert r["vert_comp"].dtype == np.int32 and r["face_comp"].dtype == np.int32
    assert np.array_equal(r["vert_comp"], comp) and np.array_equal(r["face_comp"], face_comp)
    assert np.array_equal(r["n_verts"], n_verts) and np.array_equal(r["n_faces"], n_faces)
    assert r["C"] == len(n_verts) and r["bbox_lo"] is None and r["bbox_hi"] is None
    # the synchronous restatement of the device's rounds reaches the same labels
    rounds, L = R.hook_rounds(faces, V)
    assert rounds <= 64 and np.array_equal(L, R.labels(faces, V))


def test_hand_checked_cases():
    r = R.components(*BOW_TIE)
    assert r["C"] == 1 and r["n_verts"].tolist() == [5] and r["n_faces"].tolist() == [2]
    r = R.components(*CASES["isolated_vertex"])
    assert r["vert_comp"].tolist() == [0, 0, 0, 1, 2, 2, 2, 3] and r["n_faces"].tolist() == [1, 0, 1, 0]
    r = R.components(*CASES["out_of_range"])
    assert r["face_comp"].tolist() == [0, -1, 1, 1, 1, -1]  # the faces with -1 and with V connect nothing
    assert r["vert_comp"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1] and r["n_faces"].tolist() == [1, 3]


def test_boxes_ignore_what_is_not_finite():
    faces, V = [[0, 1, 2], [3, 4, 5]], 7
    verts = np.array([[1, 2, 3], [-1, np.nan, 5], [0.5, -2, np.inf], [-0.0, 1, np.nan], [0.0, 1, np.nan], [-0.0, 1, -np.inf],
                      [np.nan, np.nan, np.nan]], np.float32)
    r = R.components(faces, V, verts)
    assert r["bbox_lo"].dtype == np.float32 and r["bbox_lo"].shape == (3, 3)
    assert r["bbox_lo"][0].tolist() == [-1, -2, 3] and r["bbox_hi"][0].tolist() == [1, 2, 5]
    assert r["bbox_lo"][1].tolist() == [0, 1, np.inf] and r["bbox_hi"][1].tolist() == [0, 1, -np.inf]
    assert not np.signbit(r["bbox_lo"][1, 0]) and not np.signbit(r["bbox_hi"][1, 0])  # -0 counts as +0
    assert r["bbox_lo"][2].tolist() == [np.inf] * 3 and r["bbox_hi"][2].tolist() == [-np.inf] * 3


def test_compaction_restatement_keeps_order_and_renumbers():
    faces, V = CASES["out_of_range"]
    verts = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    r = R.components(faces, V, verts)
    v, f, n, c = R.compact(verts, faces, r["vert_comp"], r["face_comp"], [False, True], normals=-verts)
    assert np.array_equal(v, verts[3:]) and np.array_equal(n, -verts[3:]) and c is None
    assert f.tolist() == [[0, 1, 2], [2, 3, 4], [4, 5, 6]] and f.dtype == np.int32
    v, f, _, _ = R.compact(verts, faces, r["vert_comp"], r["face_comp"], [True, True])
    assert np.array_equal(v, verts) and f.tolist() == [[0, 1, 2], [3, 4, 5], [5, 6, 7], [7, 8, 9]]  # the two bad faces go
    v, f, _, _ = R.compact(verts, faces, r["vert_comp"], r["face_comp"], [False, False])
    assert v.shape == (0, 3) and f.shape == (0, 3)


def _comps(pkg, n_faces):
    n = torch.tensor(n_faces, dtype=torch.int32)
    return pkg.mesh.Components(None, None, torch.ones_like(n), n, None, None)


def test_select_components_ties_and_combination(pkg):
    sel = pkg.mesh.select_components
    n_faces = [4, 9, 9, 0, 2, 9, 4]
    c = _comps(pkg, n_faces)
    assert sel(c).tolist() == [True, True, True, False, True, True, True]  # min_faces = 1 drops the face-less vertices
    assert sel(c, min_faces=0).all() and not sel(c, min_faces=10).any()
    assert sel(c, min_faces=4).tolist() == [True, True, True, False, False, True, True]
    assert sel(c, keep_largest=2).tolist() == [False, True, True, False, False, False, False]  # three tie at 9: the lower ids stay
    assert sel(c, keep_largest=4).tolist() == [True, True, True, False, False, True, False]  # 4 ties with 4: id 0 stays
    assert sel(c, min_faces=5, keep_largest=4).tolist() == [False, True, True, False, False, True, False]  # both conditions
    assert sel(c, min_faces=0, keep_largest=0).tolist() == [False] * 7 and sel(c, min_faces=0, keep_largest=99).all()
    for mf, k in ((1, None), (4, None), (1, 2), (1, 4), (5, 4), (0, 0), (3, 6)):
        assert sel(c, min_faces=mf, keep_largest=k).tolist() == R.select(n_faces, mf, k).tolist()
    assert sel(_comps(pkg, []), keep_largest=3).shape == (0,)
    with pytest.raises(ValueError):
        sel(c, keep_largest=-1)


def test_components_needs_a_device(pkg):
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.components(torch.zeros(2, 3, dtype=torch.int32), 4)


def test_cli_parses_component_options(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    d = ap.parse_args(["--mesh", "64"])
    assert d.mesh_min_faces is None and d.mesh_keep_largest is None
    a = ap.parse_args(["--mesh", "256", "--mesh-min-faces", "100", "--mesh-keep-largest", "3", "--mesh-band", "8"])
    assert a.mesh_min_faces == 100 and a.mesh_keep_largest == 3 and a.mesh_band == 8
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh-min-faces", "many"])
    src = open(os.path.join(ROOT, "nerf-tiny_amd", "main.py")).read()
    assert "min_faces=args.mesh_min_faces, keep_largest=args.mesh_keep_largest" in src


def test_strips_need_few_synchronous_rounds():
    """The round counts that the header and DESIGN.md section 3h-3 quote for the cap's margin."""
    strip = lambda n: np.stack([np.arange(n - 2), np.arange(n - 2) + 1, np.arange(n - 2) + 2], 1)
    assert R.hook_rounds(strip(65536), 65536)[0] == 2
    for n, want in ((4096, 8), (65536, 11)):
        perm = np.random.default_rng(0).permutation(n)
        rounds, L = R.hook_rounds(perm[strip(n)], n)
        assert rounds == want and (L == 0).all()
