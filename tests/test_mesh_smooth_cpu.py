"""CPU: the numpy restatement of the edge topology, the smoothing steps and the face normals (tests/smooth_reference.py) against a
plain-loop reading of include/nerf_hip.h, the known topology of the shared fixtures, and properties of the definition itself.  The
product's host-side pieces that need no device (the box rule, the argument errors, the refusal of CPU tensors) are held here too."""
import numpy as np
import pytest
import torch

import simplify_meshes as M
import smooth_reference as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the restatement against the loops ----

def test_patchwork_has_every_case():
    v, f = R.patchwork()
    t = R.topology(f, len(v))
    faces, E, nb, nm, ni, used, _, most = t["counts"]
    assert 30 <= len(f) <= 60 and faces == len(f) - 4  # the repeated-index face and the three out-of-range faces take no part
    assert nb > 0 and nm == 1 and ni >= 1 and used == len(v) - 1 and t["degree"][-1] == 0
    assert (t["count"] > 2).sum() == 1 and ((t["count"] == 2) & (np.abs(t["tally"]) == 2)).sum() == ni
    assert np.isnan(v).any() and np.isinf(v).any() and not t["closed"]


def test_topology_against_loops():
    for v, f in (R.patchwork(), M.fan()[:2], (M.bad_input()[0], M.bad_input()[1])):
        t = R.topology(f, len(v))
        degree, flags, counts = R.topology_loops(f, len(v))
        assert counts == t["counts"]
        assert np.array_equal(degree, t["degree"]) and np.array_equal(flags, t["vert_flags"])


@pytest.mark.parametrize("fix", [True, False])
def test_steps_against_loops(fix):
    v, f = R.patchwork()
    for lo, scale in (R.default_box(v), ((1.5, 0.25, 0.0), 1.0)):  # the second box clamps on both sides: the mesh is four units wide
        t = R.topology(f, len(v))
        cur_a = cur_b = v
        for w in (0.5, -0.53, 0.5):
            cur_a = R.step(cur_a, t, lo, scale, w, fix)
            cur_b = R.step_loops(cur_b, f, lo, scale, w, fix)
            assert np.array_equal(_bits(cur_a), _bits(cur_b))
        assert not np.array_equal(_bits(cur_a), _bits(v))
    uc, _ = R.box_coords(v, (1.5, 0.25, 0.0), 1.0)
    assert (uc == 2.0).any() and (uc == -1.0).any()


def test_normals_against_loops():
    v, f = R.patchwork()
    for lo, scale in (R.default_box(v), ((1.5, 0.25, 0.0), 1.0)):
        assert np.array_equal(_bits(R.vertex_normals(v, f, lo, scale)), _bits(R.vertex_normals_loops(v, f, lo, scale)))
    n = R.vertex_normals(v, f)
    assert (n[-1] == 0).all()  # the isolated vertex
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0))


# ---- the shared fixtures' known topology ----

def test_known_topology_of_blobs():
    v, f, _ = M.blobs()
    t = R.topology(f, len(v))
    assert (len(v), len(f)) == (1034, 2052)
    assert t["counts"] == [2052, 3078, 0, 0, 0, 1034, 0, 9]
    assert t["euler"] == 8 and t["closed"]  # four closed components of genus 0: the three balls and the island


def test_known_topology_of_the_random_mesh():
    v, f, _ = M.random_mesh()
    t = R.topology(f, len(v))
    assert (len(v), len(f)) == (5785, 10476)
    assert t["counts"][:5] == [10476, 17583, 3738, 0, 0] and t["counts"][7] == 14 and not t["closed"]


# ---- behaviour ----

def test_zero_iterations_is_the_identity():
    v, f, _ = M.bad_input()[:3]
    r = R.smooth(v, f, iterations=0)
    assert r["steps"] == 0 and np.array_equal(_bits(r["verts"]), _bits(v))


def test_pinned_and_isolated_vertices_keep_their_bits():
    v, f, _ = M.random_mesh()
    v = np.concatenate((v, [[3.0, 4.0, 5.0]])).astype(np.float32)  # a vertex in no face
    r = R.smooth(v, f, iterations=3)
    pinned = (r["topo"]["vert_flags"] & 1) != 0
    assert r["pinned"] == pinned.sum() > 1000 and r["topo"]["degree"][-1] == 0
    assert np.array_equal(_bits(r["verts"][pinned]), _bits(v[pinned])) and np.array_equal(_bits(r["verts"][-1]), _bits(v[-1]))
    moved = (_bits(r["verts"]) != _bits(v)).any(1)
    free_verts = ~pinned & (r["topo"]["degree"] > 0)
    assert not moved[~free_verts].any() and moved[free_verts].mean() > 0.99 and free_verts.sum() > 2000
    free = R.smooth(v, f, iterations=3, fix_boundary=False)
    assert free["pinned"] == 0 and (_bits(free["verts"][pinned]) != _bits(v[pinned])).any(1).sum() > 1000


def test_bad_vertices_are_skipped_and_copied():
    v, f, _ = M.bad_input()[:3]
    r = R.smooth(v, f, iterations=2, lo=(0, 0, 0), scale=16.0)
    bad = ~np.isfinite(v).all(1)
    assert bad.sum() == 40 and np.array_equal(_bits(r["verts"][bad]), _bits(v[bad]))
    assert np.isfinite(r["verts"][~bad]).all()


@pytest.mark.parametrize("name", ["blobs", "random_mesh"])
def test_a_box_that_contains_the_mesh_never_clamps(name):
    v, f, _ = getattr(M, name)()
    lo, scale = R.default_box(v)
    t = R.topology(f, len(v))
    cur, worst = v, 0.0
    for _ in range(10):
        for w in (0.5, -0.53):
            cur = R.step(cur, t, lo, scale, w)
            u = (cur.astype(np.float64) - lo.astype(np.float64)) / np.float64(scale)
            worst = max(worst, float(np.abs(u).max()))
            assert u.min() > -1.0 and u.max() < 2.0
    print(f"{name}: |uc| <= {worst:.3f} over 10 iterations (box lo {lo}, scale {scale})")
    assert worst < 1.0


def test_the_box_rule():
    assert [float(R.pow2_at_least(x)) for x in (0.0, -1.0, 1.0, 1.5, 2.0, 23.0, 0.3, np.nan)] == [1, 1, 1, 2, 2, 32, 0.5, 1]
    assert R.pow2_at_least(np.inf) == np.float32(2.0 ** 127) == R.pow2_at_least(3e38)
    lo, scale = R.default_box(np.full((4, 3), np.nan, np.float32))
    assert (lo == 0).all() and scale == 1
    lo, scale = R.default_box(np.ones((4, 3), np.float32))  # extent 0
    assert (lo == 1).all() and scale == 1


# ---- shrinkage: a property of the definition ----

def test_taubin_keeps_the_volume_and_laplace_does_not():
    """A property of the definition, on the 32^3 sphere field at level 0 (2402 vertices, closed, volume 6015.9): 20 Taubin iterations
    leave the enclosed volume within 2 %, 40 plain lambda = 0.5 steps shrink it by more than 10 %.  The restatement gives +0.51 % and
    -18.0 % (printed below), so the bounds hold with a factor of about 4 and of about 2 of margin."""
    v, f, n = R.sphere32()
    t = R.topology(f, len(v))
    assert len(v) == 2402 and t["closed"] and t["euler"] == 2
    v0 = R.volume(v, f)
    assert abs(v0 - 6015.9) < 0.1
    taubin = R.smooth(v, f, iterations=20)
    laplace = R.smooth(v, f, iterations=40, mu=None)
    d_t, d_l = R.volume(taubin["verts"], f) / v0 - 1, R.volume(laplace["verts"], f) / v0 - 1
    print(f"volume change: Taubin x 20 {100 * d_t:+.2f} %, Laplace x 40 {100 * d_l:+.2f} %")
    assert abs(d_t) < 0.02 and d_l < -0.10
    assert ((taubin["normals"] * n).sum(1) > 0.9).all()  # the face normals of the smoothed sphere agree with marching cubes'


# ---- the package's host side (no device needed) ----

def test_package_box_rule_matches(pkg):
    for x in (0.0, -1.0, 1.0, 1.5, 2.0, 23.0, 0.3, np.nan, np.inf, 3e38, 1e-40, 2.0 ** -149, 2.4):
        assert pkg.mesh.pow2_at_least(x) == R.pow2_at_least(x), x
    for v in (M.random_mesh()[0], M.bad_input()[0], np.full((4, 3), np.nan, np.float32), np.ones((4, 3), np.float32), np.zeros((0, 3), np.float32)):
        for lo in (None, (-1.0, 0.5, 0.0)):
            got, want = pkg.mesh.smooth_box(torch.from_numpy(np.array(v)), lo), R.default_box(v, lo)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[0].dtype == np.float32
    assert pkg.mesh.smooth_box(torch.zeros(3, 3), (1, 2, 3), 4.0)[1] == 4.0


def test_cpu_tensors_are_refused(pkg):
    v, f, _ = M.random_mesh()
    m = pkg.mesh.Mesh(torch.from_numpy(v.copy()), torch.from_numpy(f.copy()), None, None)
    for call in (lambda: pkg.mesh.smooth(m), lambda: pkg.mesh.topology(m.faces, len(v)), lambda: pkg.mesh.vertex_normals(m.verts, m.faces)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_main_has_the_flag(pkg):
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("nerf_main", os.path.join(ROOT, "nerf-tiny_amd", "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.build_parser().parse_args(["--mesh", "64", "--mesh-smooth", "5"])
    assert args.mesh_smooth == 5 and mod.build_parser().parse_args([]).mesh_smooth is None
