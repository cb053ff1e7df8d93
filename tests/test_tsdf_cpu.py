"""CPU: the numpy restatements of the TSDF fusion rule (tests/tsdf_reference.py; rule T of include/nerf_hip.h) agree with each other, and
the rule with its defaults does what the fusion is for -- on an analytic sphere every zero crossing of mesh.tsdf_grid lies on the sphere
and the mesh closes; with the opposite defaults a second sheet appears behind the surface."""
import numpy as np
import pytest
import torch

import mc_reference as MC
import tsdf_reference as R

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("with_opacity", [True, False])
def test_vectorised_and_loops_models_agree(carve, with_opacity):
    s = R.random_case()
    z = np.zeros(s["shape"], F32)
    op = s["opacity"] if with_opacity else None
    a = R.integrate(z, z, s["lo"], s["step"], s["depth"], op, s["cams"], s["trunc"], 0.5, carve)
    b = R.integrate_loops(z, z, s["lo"], s["step"], s["depth"], op, s["cams"], s["trunc"], 0.5, carve)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    seen = a[1] > 0
    print(f"carve {carve} opacity {with_opacity}: {int(seen.sum())} of {seen.size} voxels observed, Wt up to {a[1].max():g}, "
          f"T in [{a[0].min():.3f}, {a[0].max():.3f}]")
    assert 0 < seen.sum() and (a[0][~seen] == 0).all() and a[1].max() >= 2 and a[0].min() < 0 < a[0].max()
    # a second call continues from the state the first left, and the views one at a time give the same state
    a2 = R.integrate(a[0], a[1], s["lo"], s["step"], s["depth"][::-1], None if op is None else op[::-1], s["cams"][::-1], s["trunc"], 0.5, carve)
    b2 = R.integrate_loops(b[0], b[1], s["lo"], s["step"], s["depth"][::-1], None if op is None else op[::-1], s["cams"][::-1], s["trunc"], 0.5, carve)
    assert np.array_equal(_bits(a2[0]), _bits(b2[0])) and np.array_equal(_bits(a2[1]), _bits(b2[1]))
    t, w = z, z
    for c in range(len(s["cams"])):
        t, w = R.integrate(t, w, s["lo"], s["step"], s["depth"][c:c + 1], None if op is None else op[c:c + 1], s["cams"][c:c + 1], s["trunc"], 0.5, carve)
    assert np.array_equal(_bits(t), _bits(a[0])) and np.array_equal(_bits(w), _bits(a[1]))


def test_the_reference_camera_is_the_packages(pkg):
    s = R.random_case()
    for p in s["poses"]:
        Q, o = pkg.mesh.camera_q(p, s["K"])
        Qr, orr = R.camera_q(p, s["K"])
        assert np.array_equal(Q, Qr) and np.array_equal(o, orr)
    # and Q maps a pixel's unit ray back to its pixel
    o, u = R.unit_rays(s["poses"][0], s["K"], s["H"], s["W"])
    m = u @ R.camera_q(s["poses"][0], s["K"])[0].T
    x, y = np.meshgrid(np.arange(s["H"]), np.arange(s["W"]), indexing="ij")
    assert np.abs(m[..., 0] / m[..., 2] - x).max() < 1e-6 and np.abs(m[..., 1] / m[..., 2] - y).max() < 1e-6 and (m[..., 2] > 0).all()


def _off_sphere(G, s):
    X = R.crossings(G, R.lattice(s["lo"], s["step"], s["shape"]))
    return X, np.abs(np.linalg.norm(X, axis=1) - R.SPHERE_R) / float(s["step"].max())


def test_sphere_zero_crossings_lie_on_the_sphere(pkg):
    s = R.sphere_scene()
    T, Wt = R.sphere_fused(True)
    G = pkg.mesh.tsdf_grid(torch.from_numpy(np.array(T)), torch.from_numpy(np.array(Wt))).numpy()
    assert np.array_equal(_bits(G), _bits(R.grid(T, Wt, "solid")))
    X, off = _off_sphere(G, s)
    print(f"sphere: {len(X)} zero crossings, the farthest {off.max():.3f} lattice steps from the sphere; {int((Wt > 0).sum())} of {Wt.size} voxels observed")
    assert len(X) >= 1 and off.max() <= 1.0
    v, f, n = MC.marching_cubes(G, 0.0, s["lo"], s["step"])
    closed, euler, vol, area = MC.mesh_stats(v, f)
    print(f"sphere mesh: V {len(v)} F {len(f)} closed {closed} euler {euler} volume {vol:.4f} (sphere {4 / 3 * np.pi * R.SPHERE_R ** 3:.4f})")
    assert closed and euler == 2 and len(f) > 100
    assert abs(vol - 4 / 3 * np.pi * R.SPHERE_R ** 3) < 0.1 * 4 / 3 * np.pi * R.SPHERE_R ** 3
    # the normals of the negated volume point outward
    assert (np.einsum("ij,ij->i", n, v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.8).all()


def test_the_opposite_defaults_leave_a_shell_behind_the_surface(pkg):
    s = R.sphere_scene()
    T, Wt = R.sphere_fused(False)
    G = pkg.mesh.tsdf_grid(torch.from_numpy(np.array(T)), torch.from_numpy(np.array(Wt)), unseen="empty").numpy()
    assert np.array_equal(_bits(G), _bits(R.grid(T, Wt, "empty")))
    X, off = _off_sphere(G, s)
    print(f"unseen=empty, carve=False: {len(X)} crossings, {int((off > 2).sum())} farther than 2 steps from the sphere")
    assert (off > 2.0).any() and (off <= 1.0).any()
    with pytest.raises(ValueError, match="unseen"):
        pkg.mesh.tsdf_grid(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2), unseen="hollow")


def test_cpu_tensors_raise_and_the_constants_agree(pkg):
    import re

    from conftest import ROOT

    hdr = open(ROOT + "/include/nerf_hip.h").read()
    assert int(re.search(r"#define NERF_HIP_TSDF_VIEWS_PER_LAUNCH (\d+)", hdr).group(1)) == pkg._abi.TSDF_VIEWS_PER_LAUNCH
    assert int(re.search(r"#define NERF_HIP_TSDF_CARVE (\d+)", hdr).group(1)) == pkg._abi.TSDF_CARVE
    s = R.random_case()
    z = torch.zeros(s["shape"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_integrate(z, z.clone(), s["lo"], s["step"], torch.from_numpy(s["depth"]), s["poses"], s["K"], trunc=s["trunc"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_volume(s["shape"], "cpu")


def test_cli_parses_mesh_tsdf(pkg):
    import importlib

    ap = importlib.import_module("nerf_tiny_amd.main").build_parser()
    a = ap.parse_args(["--mesh", "32", "--mesh-tsdf"])
    assert a.mesh_tsdf == "train" and a.mesh_tsdf_trunc is None and a.mesh_tsdf_every == 1
    a = ap.parse_args(["--mesh", "32", "--mesh-tsdf", "val", "--mesh-tsdf-trunc", "0.05", "--mesh-tsdf-every", "3"])
    assert (a.mesh_tsdf, a.mesh_tsdf_trunc, a.mesh_tsdf_every) == ("val", 0.05, 3)
    assert ap.parse_args(["--mesh", "32"]).mesh_tsdf is None
