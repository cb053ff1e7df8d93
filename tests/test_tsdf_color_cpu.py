"""CPU: the numpy restatements of rules TC, S and M (tests/tsdf_color_reference.py) against each other and on the analytic sphere of
tests/tsdf_reference.py -- what colour fusion and masked marching cubes promise, without a device."""
import numpy as np

import mc_reference as MC
import tsdf_color_reference as RC
import tsdf_reference as R

F32 = np.float32


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _mixed(G):
    """[nx - 1, ny - 1, nz - 1] bool: the cells with corners on both sides of 0"""
    nx, ny, nz = G.shape
    ins = [(G > 0)[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] for dx, dy, dz in MC.CORNERS]
    return np.any(ins, 0) & ~np.all(ins, 0)


# ---- the two restatements of each rule agree bit for bit ----

def test_tc_restatements_agree_and_keep_rule_t():
    for carve, with_opacity in ((True, True), (False, True), (True, False)):
        s = R.random_case()
        rgb = RC.random_rgb(s)
        z, zc = np.zeros(s["shape"], F32), np.zeros(s["shape"] + (4,), F32)
        op = s["opacity"] if with_opacity else None
        args = (s["lo"], s["step"], s["depth"], op, rgb, s["cams"], s["trunc"], 0.5, carve)
        a = RC.integrate_color(z, z, zc, *args)
        b = RC.integrate_color_loops(z, z, zc, *args)
        t = R.integrate(z, z, s["lo"], s["step"], s["depth"], op, s["cams"], s["trunc"], 0.5, carve)
        assert all(_bits(x, y) for x, y in zip(a, b))
        assert _bits(a[0], t[0]) and _bits(a[1], t[1])
        wc = a[2][..., 3]
        assert (wc > 0).any() and (wc >= 2).any() and (wc <= a[1]).all() and (wc < a[1]).any() and np.isfinite(a[2]).all()
        assert not a[2][wc == 0].any()
        # a second call continues from the state (the views reversed)
        rev = slice(None, None, -1)
        args2 = (s["lo"], s["step"], s["depth"][rev], None if op is None else op[rev], rgb[rev], s["cams"][rev], s["trunc"], 0.5, carve)
        a2, b2 = RC.integrate_color(*a, *args2), RC.integrate_color_loops(*b, *args2)
        assert all(_bits(x, y) for x, y in zip(a2, b2)) and not _bits(a2[2], a[2])


def test_s_restatements_agree():
    for shape in ((5, 6, 7), (1, 6, 7)):
        C = RC.random_color_volume(shape)
        lo, step = np.array([-1.0, -0.9, -1.1], F32), np.array([0.5, 0.36, 0.37], F32)
        pts = sample_points(shape, lo, step)
        rgb, valid = RC.sample_color(C, lo, step, pts)
        rgb2, valid2 = RC.sample_color_loops(C, lo, step, pts)
        assert _bits(rgb, rgb2) and np.array_equal(valid, valid2) and valid.any() and (~valid).any()
        assert not rgb[~valid].any() and not valid[~np.isfinite(pts).all(1)].any()
    # exactly on a lattice point with a colour: that colour
    C = RC.random_color_volume((5, 6, 7))
    P = R.lattice(lo, step, (5, 6, 7))
    has = C[..., 3] > 0
    rgb, valid = RC.sample_color(C, lo, step, P[has])
    assert valid.all() and np.abs(rgb - C[has][:, :3]).max() < 1e-5


def sample_points(shape, lo, step, n=1000, seed=3):
    """the points of the S tests: inside, on lattice points, on the box faces, outside, not finite, and inside one all-empty cell"""
    rng = np.random.default_rng(seed)
    hi = lo + step * (np.asarray(shape, F32) - 1)
    pts = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(F32)
    pts[:300] = rng.uniform(lo, hi, (300, 3)).astype(F32)
    P = R.lattice(lo, step, shape).reshape(-1, 3)
    pts[300:400] = P[rng.integers(0, len(P), 100)]
    pts[400:450, 0], pts[450:500, 2] = lo[0], hi[2]
    pts[500:510, 1] = np.nan
    pts[510:520, 0] = np.inf
    pts[520:530, 2] = -np.inf
    pts[530:540] = [1e30, -1e30, 3e38]
    return pts


def test_m_restatements_agree():
    table = MC.load_table()
    for shape, seed in (((6, 7, 8), 11), ((5, 5, 9), 12)):
        g, valid = RC.random_grid_and_mask(shape, seed, 0.9)
        lo, step = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125)
        a = RC.marching_cubes_masked(g, valid, 0.1, lo, step, table)
        b = RC.marching_cubes_masked_loops(g, valid, 0.1, lo, step, table)
        full = MC.marching_cubes(g, 0.1, lo, step, table)
        assert all(_bits(x, y) for x, y in zip(a, b))
        assert 0 < len(a[1]) < len(full[1]) and 0 < len(a[0]) < len(full[0])
        assert np.array_equal(np.unique(a[1]), np.arange(len(a[0])))  # every vertex is referenced
        ones = np.ones(shape, bool)
        assert all(_bits(x, y) for x, y in zip(RC.marching_cubes_masked(g, ones, 0.1, lo, step, table), full))
        assert all(_bits(x, y) for x, y in zip(RC.marching_cubes_masked_loops(g, ones, 0.1, lo, step, table), full))
        assert all(len(x) == 0 for x in RC.marching_cubes_masked(g, ~ones, 0.1, lo, step, table))


# ---- the sphere scene ----

def test_sphere_masked_is_the_solid_mesh_when_carving():
    s = R.sphere_scene()
    T, Wt = R.sphere_fused(True)
    solid, empty = R.grid(T, Wt, "solid"), R.grid(T, Wt, "empty")
    live = RC.live_cells(Wt > 0)
    ms, me = _mixed(solid), _mixed(empty)
    print(f"mixed cells: solid {int(ms.sum())} (live {int((ms & live).sum())}), empty {int(me.sum())} (live {int((me & live).sum())})")
    assert ms.sum() == 1026 and (ms & live).sum() == 1026 and (me & ~ms).sum() == 194 and not (me & ~ms & live).any()
    want = MC.marching_cubes(solid, 0.0, s["lo"], s["step"])
    got = RC.marching_cubes_masked(empty, Wt > 0, 0.0, s["lo"], s["step"])
    assert _bits(got[0], want[0]) and _bits(got[1], want[1])
    off = np.abs(np.linalg.norm(got[0].astype(np.float64), axis=1) - R.SPHERE_R) / float(s["step"].max())
    closed, euler, _, _ = MC.mesh_stats(got[0], got[1])
    print(f"masked sphere: V {len(got[0])} F {len(got[1])}, farthest vertex {off.max():.3f} steps, closed {closed}, Euler {euler}")
    assert len(got[0]) == 1024 and off.max() < 0.53 and closed and euler == 2
    # the unmasked empty grid has the second sheet: 192 crossings more
    assert len(MC.marching_cubes(empty, 0.0, s["lo"], s["step"])[0]) == 1024 + 192


def test_sphere_masked_without_carving_is_open():
    s = R.sphere_scene()
    T, Wt = R.sphere_fused(False)
    solid, empty = R.grid(T, Wt, "solid"), R.grid(T, Wt, "empty")
    valid = Wt > 0
    live = RC.live_cells(valid)
    ms, me = _mixed(solid), _mixed(empty)
    print(f"carve=False mixed cells: empty {int(me.sum())}, solid {int(ms.sum())}, live and mixed {int((me & live).sum())}")
    assert (me & live).sum() == 1016 and (ms & live).sum() == 1016 and me.sum() == 1340 and ms.sum() == 3414
    v, f, _ = RC.marching_cubes_masked(empty, valid, 0.0, s["lo"], s["step"])
    cells = RC.face_cells(empty, 0.0)
    assert len(f) == int(live.reshape(-1)[cells].sum()) and np.array_equal(np.unique(f), np.arange(len(v)))
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, cnt = np.unique(d, axis=0, return_counts=True)
    off = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R.SPHERE_R) / float(s["step"].max())
    print(f"carve=False masked sphere: V {len(v)} F {len(f)}, boundary edges {int((cnt == 1).sum())}, {int((off > 0.53).sum())} crossings beyond "
          f"0.53 steps, the farthest {off.max():.3f}")
    assert (cnt == 1).sum() > 0 and (cnt <= 2).all()


def test_sphere_fused_colours():
    s = R.sphere_scene()
    T, Wt, C = RC.sphere_fused_color(True)
    plain = R.sphere_fused(True)
    assert _bits(T, plain[0]) and _bits(Wt, plain[1])
    v, f, _ = RC.marching_cubes_masked(R.grid(T, Wt, "empty"), Wt > 0, 0.0, s["lo"], s["step"])
    rgb, valid = RC.sample_color(C, s["lo"], s["step"], v)
    assert len(v) == 1024 and valid.all()
    p = v.astype(np.float64)
    want = 0.5 + 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True)
    err = np.abs(rgb.astype(np.float64) - want)
    print(f"fused colours at the {len(v)} vertices: worst channel error {err.max():.4f}, mean {err.mean():.4f}; "
          f"{int((C[..., 3] > 0).sum())} of {C[..., 3].size} lattice points have a colour")
    assert err.max() < 0.10
