"""GPU: marching cubes on the device (nerf_hip_mesh_count / nerf_hip_mesh_emit, ops / mesh.marching_cubes, NeRFModel.extract_mesh,
NeRFRunner.extract_mesh) against the numpy restatement in tests/mc_reference.py, bit for bit; closed, outward surfaces on smooth
fields; and stores that stay inside the caller's capacities."""
import ctypes
import glob

import numpy as np
import pytest
import torch

import mc_reference as R
from test_mesh_cpu import _read_ply

pytestmark = pytest.mark.gpu


def _check_against_reference(pkg, dev, s, level, lo=(0, 0, 0), step=(1, 1, 1)):
    v, f, n = pkg.mesh.marching_cubes(torch.from_numpy(s).to(dev), level, lo, step)
    rv, rf, rn = R.marching_cubes(s, level, lo, step)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    assert v.shape == rv.shape and f.shape == rf.shape and n.shape == rn.shape
    assert np.array_equal(v.view(np.int32), rv.view(np.int32))  # bit-identical (NaN-free: every vertex is finite here)
    assert np.array_equal(f, rf)
    if len(n):
        assert np.abs(n - rn).max() <= 1e-6
    return v, f, n


def _cube_rows(s, level):
    inside = s > level
    nx, ny, nz = s.shape
    cube = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (dx, dy, dz) in enumerate(R.CORNERS):
        cube |= (~inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]).astype(np.int64) << c
    return np.unique(cube)


@pytest.mark.parametrize("shape", [(1, 5, 5), (2, 2, 2), (3, 70, 129), (64, 64, 64), (257, 256, 255)])
def test_random_grids_match_the_reference(pkg, dev, shape):
    s = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)
    v, f, n = _check_against_reference(pkg, dev, s, 0.5)
    if shape == (1, 5, 5):
        assert v.shape == (0, 3) and f.shape == (0, 3)
    if np.prod([d - 1 for d in shape]) >= 20000:
        assert len(_cube_rows(s, 0.5)) == 256  # every table row is exercised
    if shape == (257, 256, 255):
        assert len(v) > 1 << 24 and len(f) > 1 << 24  # many workgroups, a long scan of block totals


def test_nan_inf_and_world_lattice(pkg, dev):
    rng = np.random.default_rng(7)
    s = rng.random((33, 40, 47), dtype=np.float32)
    flat = s.reshape(-1)
    pick = rng.choice(flat.size, 600, replace=False)
    flat[pick[:200]] = np.nan
    flat[pick[200:400]] = np.inf
    flat[pick[400:]] = -np.inf
    lo = (-1.25, 0.5, 3.0)
    step = (np.float32(0.03), np.float32(0.07), np.float32(0.011))
    v, f, n = _check_against_reference(pkg, dev, s, 0.5, lo, step)
    assert len(f) > 0 and (n == 0).all(axis=1).any()  # gradients through inf / NaN give the zero normal
    _check_against_reference(pkg, dev, s, -0.25, lo, step)  # every finite value inside


def _lattice(shape, lo, step):
    axes = [np.float32(lo[c]) + np.arange(shape[c], dtype=np.float32) * np.float32(step[c]) for c in range(3)]
    return np.meshgrid(*axes, indexing="ij")


@pytest.mark.parametrize("shape", [(128, 128, 128), (96, 128, 112)])
def test_sphere_is_closed_and_outward(pkg, dev, shape):
    h = np.float32(2.0 / 127)
    lo = [-np.float32(h * (n - 1) / 2) for n in shape]
    X, Y, Z = _lattice(shape, lo, (h, h, h))
    Rs, level = 30.5 * float(h), 10.0  # isosurface radius 30.5 cells
    sig = (100 * np.maximum(0, Rs + level / 100 - np.sqrt(X.astype(np.float64) ** 2 + Y ** 2 + Z ** 2))).astype(np.float32)
    v, f, n = _check_against_reference(pkg, dev, sig, level, lo, (h, h, h))
    closed, chi, vol, area = R.mesh_stats(v, f)
    assert closed and chi == 2
    assert vol > 0 and abs(vol / (4 / 3 * np.pi * Rs ** 3) - 1) < 0.01
    assert abs(area / (4 * np.pi * Rs ** 2) - 1) < 0.01
    # normals point away from the centre
    assert (np.einsum("ij,ij->i", n.astype(np.float64), v.astype(np.float64)) > 0).all()


@pytest.mark.parametrize("shape", [(128, 128, 128), (128, 100, 128)])
def test_torus_is_closed_and_outward(pkg, dev, shape):
    h = np.float32(2.0 / 127)
    lo = [-np.float32(h * (n - 1) / 2) for n in shape]
    X, Y, Z = _lattice(shape, lo, (h, h, h))
    ring, tube, level = 0.55, 22.5 * float(h), 10.0  # tube radius 22.5 cells, in the x-z plane
    d = np.sqrt((np.sqrt(X.astype(np.float64) ** 2 + Z ** 2) - ring) ** 2 + Y.astype(np.float64) ** 2)
    sig = (100 * np.maximum(0, tube + level / 100 - d)).astype(np.float32)
    v, f, n = _check_against_reference(pkg, dev, sig, level, lo, (h, h, h))
    closed, chi, vol, area = R.mesh_stats(v, f)
    assert closed and chi == 0
    assert vol > 0 and abs(vol / (2 * np.pi ** 2 * ring * tube ** 2) - 1) < 0.01


def _model(pkg, oracle, dev, seed, sharp):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(seed, sharp))
    return m.to(dev)


@pytest.mark.parametrize("sharp", [False, True])
def test_model_extract_mesh_is_the_composition(oracle, pkg, dev, sharp):
    m = _model(pkg, oracle, dev, 5, sharp)
    lo, hi, shape = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), (37, 20, 45)
    grid = m.density_grid(lo, hi, shape)
    level = float(grid.median())
    from nerf_tiny_amd.nerf import grid_step

    step = grid_step(np.float32(lo), np.float32(hi), shape)
    v, f, n = pkg.mesh.marching_cubes(grid, level, lo, step)
    rgb, _ = m.query(v, -n)
    m.bf16_mlp = sharp  # the model's flags do not apply
    out = m.extract_mesh(lo, hi, shape, level)
    assert len(out.faces) > 100
    for a, b in zip(out, (v, f, n, rgb)):
        assert a.device == grid.device and torch.equal(a, b)
    plain = m.extract_mesh(lo, hi, shape, level, color=False)
    assert plain.rgb is None
    for a, b in zip(plain[:3], (v, f, n)):
        assert torch.equal(a, b)
    rv, rf, _ = R.marching_cubes(grid.cpu().numpy(), level, lo, step)
    assert np.array_equal(out.verts.cpu().numpy(), rv) and np.array_equal(out.faces.cpu().numpy(), rf)


def test_runner_exports_a_mesh(pkg, dev, tmp_path):
    scene = pkg.data.synthetic_scene(n_pic=4, H=32, W=32, seed=1)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=6, batch_ray=256, learning=3e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1000, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1000)
    run = pkg.NeRFRunner(continue_=False, **kw)
    assert run.trainer("train") == 5
    sig = run.density_grid(32, save=False)
    level = float(np.median(sig))
    out = run.extract_mesh(32, level, save=True)
    files = glob.glob(rs + "*_5_mesh32.ply")
    assert len(files) == 1
    assert len(out.faces) > 0 and out.rgb.shape == out.verts.shape
    _, V, F = _read_ply(files[0])
    assert np.array_equal(np.stack([V["x"], V["y"], V["z"]], 1), out.verts)
    assert np.array_equal(np.stack([V["nx"], V["ny"], V["nz"]], 1), out.normals)
    assert np.array_equal(np.stack([V["red"], V["green"], V["blue"]], 1), np.clip(np.rint(out.rgb.astype(np.float64) * 255), 0, 255))
    assert np.array_equal(F["i"], out.faces)
    from nerf_tiny_amd.nerf import grid_step

    lo = np.float32([-1.5] * 3)
    rv, rf, _ = R.marching_cubes(sig, level, lo, grid_step(lo, -lo, (32, 32, 32)))
    assert np.array_equal(out.verts, rv) and np.array_equal(out.faces, rf)
    run.rank = 1  # under a launcher only rank 0 computes and writes
    assert run.extract_mesh(32, level, save=True) is None
    assert len(glob.glob(rs + "*_mesh32.ply")) == 1


def test_emit_stays_inside_its_capacities(pkg, dev):
    L = pkg._abi.lib()
    shape = (40, 50, 60)
    s = torch.from_numpy(np.random.default_rng(2).random(shape, dtype=np.float32)).to(dev)
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    v_full, f_full, n_full = pkg.mesh.marching_cubes(s, 0.5)
    V, F = len(v_full), len(f_full)
    ws = torch.empty(pkg._abi.mesh_ws_bytes(*shape), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    GUARD = 4096
    for level_emit, cap_v, cap_f in ((0.5, V // 2, F // 3), (0.5, 0, F // 2), (0.5, V, 0), (0.3, V, F)):
        # (0.3: an emit that does not match its count -- more vertices and faces than the capacities: wrong output, bounded stores)
        pkg._abi.check(L.nerf_hip_mesh_count(s.data_ptr(), *shape, 0.5, ws.data_ptr(), ws.numel(), counts.data_ptr(), st))
        verts = torch.full((cap_v + GUARD, 3), 7.25, device=dev)
        normals = torch.full((cap_v + GUARD, 3), -3.5, device=dev)
        faces = torch.full((cap_f + GUARD, 3), -77, dtype=torch.int32, device=dev)
        pkg._abi.check(L.nerf_hip_mesh_emit(s.data_ptr(), *shape, lo, step, level_emit, ws.data_ptr(), ws.numel(), verts.data_ptr(),
                                            normals.data_ptr(), faces.data_ptr(), cap_v, cap_f, st))
        torch.cuda.synchronize()
        assert counts.tolist() == [V, F]
        assert (verts[cap_v:] == 7.25).all() and (normals[cap_v:] == -3.5).all() and (faces[cap_f:] == -77).all()
        if level_emit == 0.5:
            assert torch.equal(verts[:cap_v], v_full[:cap_v]) and torch.equal(faces[:cap_f], f_full[:cap_f])
            assert torch.equal(normals[:cap_v], n_full[:cap_v])


def test_host_refusals_launch_nothing(pkg, dev):
    L = pkg._abi.lib()
    shape = (8, 8, 8)
    s = torch.rand(shape, device=dev)
    ws = torch.empty(pkg._abi.mesh_ws_bytes(*shape), dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -5, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    out = torch.full((64, 3), 9.0, device=dev)
    fo = torch.full((64, 3), 9, dtype=torch.int32, device=dev)

    def rc_count(*dims, level=0.5, nbytes=ws.numel()):
        return L.nerf_hip_mesh_count(s.data_ptr(), *dims, level, ws.data_ptr(), nbytes, counts.data_ptr(), st)

    def rc_emit(*dims, level=0.5, stp=step, nbytes=ws.numel()):
        return L.nerf_hip_mesh_emit(s.data_ptr(), *dims, lo, stp, level, ws.data_ptr(), nbytes, out.data_ptr(), out.data_ptr(),
                                    fo.data_ptr(), 64, 64, st)

    assert rc_count(*shape, nbytes=ws.numel() - 256) == -2 and rc_emit(*shape, nbytes=ws.numel() - 256) == -2
    assert rc_count(0, 8, 8) == -1 and rc_emit(8, 0, 8) == -1
    assert rc_count(*shape, level=float("nan")) == -1 and rc_emit(*shape, level=float("inf")) == -1
    assert rc_emit(*shape, stp=pkg._abi.f32_array([1, -1, 1])) == -1
    torch.cuda.synchronize()
    assert (counts == -5).all() and (out == 9.0).all() and (fo == 9).all()
    # grids with a dimension of one point: the empty mesh, counted on the device
    assert L.nerf_hip_mesh_count(s.data_ptr(), 1, 8, 64, 0.5, ws.data_ptr(), ws.numel(), counts.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
