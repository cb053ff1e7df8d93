"""CPU: the SH radiance volume rules restated in numpy (tests/volume_reference.py) hold together -- the quadrature, the occupancy, the
block skip, the stated bound and its teeth -- before any kernel is asked to match them."""
import numpy as np
import pytest

import volume_reference as R

F = np.float32
SHAPE = (9, 8, 7)
NRAYS = 300
DT = F(0.04)           # the box's diagonal is 2.83: at most 71 samples a ray
BG = (0.25, 0.5, 1.0)


@pytest.fixture(scope="module")
def scene():
    sigma, coef, lo, step = R.make_volume(SHAPE, seed=11)
    o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, SHAPE)
    out = {}
    for name, B in (("1", 1), ("2", 2), ("4", 4), ("one", 1 << 20)):
        occ = R.blocks(sigma, B)
        out[name] = R.march(sigma, coef, occ, B, lo, step, o, d, tmin, tmax, DT, 0.0, BG)
    return dict(sigma=sigma, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax, out=out)


def test_library_tables_are_the_rule(pkg):
    dirs, b = R.sh_tables()
    ld, lb = pkg._abi.volume_sh_table()
    assert np.array_equal(np.asarray(ld, F).view(np.uint32), dirs.view(np.uint32))
    assert np.array_equal(np.asarray(lb, F).view(np.uint32), b.view(np.uint32))
    # the basis constants: the header's macro is the one copy the kernels and the host tables are built from
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    macro = re.search(r"#define NERF_HIP_VOLUME_SH_C \{([^}]*)\}", src).group(1)
    header = np.asarray([float(x.strip().rstrip("f")) for x in macro.split(",")], F)
    assert np.array_equal(np.asarray(R.SH_C32, F).view(np.uint32), header.view(np.uint32))


def test_quadrature_is_exact_to_degree_two():
    dirs, b = R.sh_tables()
    d64 = dirs.astype(np.float64)
    Y = R.basis64(d64)
    G = (4 * np.pi / 12) * Y.T @ Y
    assert np.abs(G - np.eye(9)).max() < 4e-7          # fp32 directions: their norm is 1 to 6e-8, squared in the products
    # a random function of degree <= 2: its coefficients come back through the fp32 table to rounding
    rng = np.random.default_rng(0)
    c = rng.normal(size=9)
    got = b.astype(np.float64).T @ (Y @ c)
    assert np.abs(got - c).max() < 1e-6 * np.abs(c).max() * 9
    # degree-3 terms leak nothing into degree <= 2 (a 5-design integrates degree 3 + 2 exactly): x y z, and z (5 z^2 - 3)
    x, y, z = d64.T
    for f3 in (x * y * z, z * (5 * z * z - 3), x * (x * x - 3 * y * y)):
        assert np.abs(b.astype(np.float64).T @ f3).max() < 4e-7


def test_occupancy_and_active_agree(scene):
    sigma = scene["sigma"]
    act = np.zeros(sigma.size, bool)
    act[R.active(sigma)] = True
    act = act.reshape(sigma.shape)
    pos = sigma > 0
    nx, ny, nz = sigma.shape
    cellpos = np.zeros((nx - 1, ny - 1, nz - 1), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cellpos |= pos[di:di + nx - 1, dj:dj + ny - 1, dk:dk + nz - 1]
    want = np.zeros(sigma.shape, bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                want[di:di + nx - 1, dj:dj + ny - 1, dk:dk + nz - 1] |= cellpos
    assert np.array_equal(act, want) and 0 < act.sum() < act.size
    # blocks of one cell are the cells; a coarser block is the OR of its cells; one block is any()
    assert np.array_equal(R.blocks(sigma, 1).astype(bool), cellpos)
    assert R.blocks(sigma, 1 << 20).shape == (1, 1, 1) and R.blocks(sigma, 1 << 20)[0, 0, 0] == 1
    o2 = R.blocks(sigma, 2)
    assert o2.shape == (4, 4, 3) and 0 < o2.sum() < o2.size


def test_inputs_exercise_the_rule(scene):
    rgb, maps, steps, info = scene["out"]["one"]
    miss = np.asarray([s is None for s, _ in info])
    assert (steps[:, 0] >= 3).sum() >= NRAYS // 2
    assert miss.sum() >= NRAYS // 10
    lo, step = scene["lo"], scene["step"]
    hi = lo + (np.asarray(SHAPE) - 1).astype(F) * step
    o, d = scene["o"], scene["d"]
    assert ((o >= lo) & (o <= hi)).all(axis=1).any() and steps[1, 0] > 0      # starts inside
    assert ((d == 0).any(axis=1) & ~miss).any() and steps[2, 0] >= 3           # a zero component, and it hits
    assert o[3, 2] == hi[2] and d[3, 2] == 0 and not miss[3]                  # lies in a face
    assert miss[4] and scene["tmin"][4] > 0                                    # window beyond the exit
    assert np.isnan(o[0]).any() and miss[0]
    assert np.array_equal(rgb[miss], np.broadcast_to(np.asarray(BG, F), rgb[miss].shape))
    assert not maps[miss].any() and not steps[miss].any()


def test_block_size_changes_only_evaluated(scene):
    ref = scene["out"]["one"]
    for name in ("1", "2", "4"):
        rgb, maps, steps, _ = scene["out"][name]
        assert np.array_equal(rgb.view(np.uint32), ref[0].view(np.uint32)), name
        assert np.array_equal(maps.view(np.uint32), ref[1].view(np.uint32)), name
        assert np.array_equal(steps[:, 0], ref[2][:, 0]), name
        assert (steps[:, 1] <= ref[2][:, 1]).all() and steps[:, 1].sum() < ref[2][:, 1].sum(), name


def _errors(scene, rgb, maps, info, dt=None):
    """per contributing ray: (error / bound) of the worst output against the fp64 composite"""
    out = []
    bgmax = max(abs(x) for x in BG)
    for r, (s, used) in enumerate(info):
        if s is None or not used:
            continue
        c64, m64 = R.composite64(s, used, BG, dt=dt)
        b = R.bound(len(used))
        tmax = max(1.0, float(np.max(s["tk"][used])))
        e = max(np.abs(rgb[r] - c64).max() / (b * (1 + bgmax)), abs(maps[r, 1] - m64[1]) / b, abs(maps[r, 0] - m64[0]) / (b * tmax))
        out.append(e)
    return np.asarray(out)


def test_fp32_march_meets_the_bound(scene):
    rgb, maps, steps, info = scene["out"]["2"]
    e = _errors(scene, rgb, maps, info)
    print(f"fp32 restatement vs fp64 composite: worst error / bound = {e.max():.3f} over {e.size} rays")
    assert e.size >= NRAYS // 2 and e.max() <= 1.0


def test_the_bound_has_teeth(scene):
    _, _, _, info = scene["out"]["one"]
    lo, step = scene["lo"], scene["step"]
    # one contributing sample dropped from the fp32 march
    rgb, maps = np.zeros((NRAYS, 3), F), np.zeros((NRAYS, 2), F)
    for r, (s, used) in enumerate(info):
        if s is not None and used:
            rgb[r], maps[r], _, _ = R.composite32(s, range(s["K"]), 0.0, BG, drop=len(used) // 2)
    e = _errors(scene, rgb, maps, info)
    assert (e > 1.0).sum() * 2 >= e.size, (e > 1.0).mean()
    # dt of the compositing scaled by (1 + 2^-10), samples unchanged
    rgb2, maps2, _, _ = scene["out"]["one"]
    e = _errors(scene, rgb2, maps2, info, dt=np.float64(DT) * (1 + 2.0 ** -10))
    assert (e > 1.0).sum() * 2 >= e.size, (e > 1.0).mean()


def test_analytic_slab():
    sigma, coef, lo, step, o, d, tmin, tmax, dt, K, sigma0, c = R.slab_case()
    occ = R.blocks(sigma, 2)
    rgb, maps, steps, _ = R.march(sigma, coef, occ, 2, lo, step, o, d, tmin, tmax, dt, 0.0, (0, 0, 0))
    R.check_slab(rgb, maps, steps, K, sigma0, c, dt)


def test_t_stop_bound(scene):
    sigma, coef, lo, step = (scene[k] for k in ("sigma", "coef", "lo", "step"))
    occ = R.blocks(sigma, 2)
    ref = scene["out"]["2"]
    n = 60
    for t_stop in (1e-3, 0.3):
        rgb, maps, steps, _ = R.march(sigma, coef, occ, 2, lo, step, scene["o"][:n], scene["d"][:n], scene["tmin"][:n], scene["tmax"][:n], DT,
                                      t_stop, BG)
        lim = t_stop * (1 + max(abs(x) for x in BG))
        assert np.abs(rgb.astype(np.float64) - ref[0][:n]).max() <= lim
        assert (steps[:, 0] <= ref[2][:n, 0]).all()
    assert (steps[:, 0] < ref[2][:n, 0]).any()


def test_driver_options():
    import importlib

    ap = importlib.import_module("nerf_tiny_amd.main").build_parser()
    a = ap.parse_args(["--volume", "48", "--volume-degree", "1", "--volume-sigma-min", "0.5", "--volume-preview"])
    assert (a.volume, a.volume_degree, a.volume_sigma_min, a.volume_preview) == (48, 1, 0.5, "test")
    a = ap.parse_args(["--volume", "32", "--volume-preview", "val"])
    assert (a.volume, a.volume_degree, a.volume_sigma_min, a.volume_preview) == (32, 2, 0.0, "val")
    a = ap.parse_args([])
    assert a.volume is None and a.volume_preview is None
    with pytest.raises(SystemExit):
        ap.parse_args(["--volume", "8", "--volume-degree", "3"])
