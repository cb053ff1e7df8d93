"""GPU: masked marching cubes on the device (nerf_hip_mesh_count_masked / nerf_hip_mesh_emit_masked, mesh.marching_cubes(valid=); rule M
of include/nerf_hip.h) against the numpy restatement in tests/tsdf_color_reference.py and against mesh.filter_faces of the unmasked
mesh, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import tsdf_color_reference as RC

pytestmark = pytest.mark.gpu
F32 = np.float32

SHAPE = (17, 18, 19)  # 5,814 points: two scan blocks of 4,096, so vertex ids cross a block boundary
LO, STEP, LEVEL = (-1.0, 0.5, 2.0), (0.25, 0.5, 0.125), 0.1


@functools.lru_cache(maxsize=None)
def _case():
    """the grid, the mask (about 95 % valid) and the restatement's masked mesh, computed once (read-only)"""
    g, valid = RC.random_grid_and_mask(SHAPE, 11, 0.95)
    want = RC.marching_cubes_masked(g, valid, LEVEL, LO, STEP)
    for a in (g, valid) + want:
        a.setflags(write=False)
    return g, valid, want


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(t, a):
    """a device tensor and a numpy array of the same 4-byte type, bit for bit"""
    a = np.array(a)  # (a copy: the shared case is read-only)
    return tuple(t.shape) == a.shape and torch.equal(t.cpu().contiguous().view(torch.int32), torch.from_numpy(a.view(np.int32)))


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _run(pkg, dev, g, valid):
    return pkg.mesh.marching_cubes(_t(g, dev), LEVEL, LO, STEP, valid=_t(valid, dev))


def test_random_mask_matches_the_restatement_and_filter_faces(pkg, dev):
    g, valid, want = _case()
    v, f, n = _run(pkg, dev, g, valid)
    full = pkg.mesh.marching_cubes(_t(g, dev), LEVEL, LO, STEP)
    print(f"masked {SHAPE}: V {len(v)} F {len(f)} of the unmasked V {len(full[0])} F {len(full[1])}; "
          f"normals differ from the restatement by at most {float(np.abs(n.cpu().numpy() - want[2]).max()):.3g}")
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and n.dtype == torch.float32
    assert 0 < len(want[1]) < len(full[1]) and 0 < len(want[0]) < len(full[0]) and np.prod(SHAPE) > 4096
    assert _bits(v, want[0]) and _bits(f, want[1]) and _bits(n, want[2])
    keep = RC.live_cells(valid).reshape(-1)[RC.face_cells(g, LEVEL)]
    assert len(keep) == len(full[1])
    m = pkg.mesh.filter_faces(pkg.mesh.Mesh(full[0], full[1], full[2], None), _t(keep, dev))
    assert _same(v, m.verts) and _same(f, m.faces) and _same(n, m.normals)
    assert torch.equal(torch.unique(f.long()), torch.arange(len(v), device=dev))  # every vertex is referenced
    again = _run(pkg, dev, g, valid)
    assert all(_same(a, b) for a, b in zip((v, f, n), again))  # two runs are identical
    # a uint8 mask with other non-zero values is the same mask
    u8 = pkg.mesh.marching_cubes(_t(g, dev), LEVEL, LO, STEP, valid=_t(valid.astype(np.uint8) * 200, dev))
    assert all(_same(a, b) for a, b in zip((v, f, n), u8))


def test_all_valid_and_all_invalid(pkg, dev):
    g, _, _ = _case()
    full = pkg.mesh.marching_cubes(_t(g, dev), LEVEL, LO, STEP)
    ones = _run(pkg, dev, g, np.ones(SHAPE, bool))
    assert len(full[1]) > 0 and all(_same(a, b) for a, b in zip(ones, full))
    v, f, n = _run(pkg, dev, g, np.zeros(SHAPE, bool))
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


def test_one_invalid_point_removes_its_eight_cells(pkg, dev):
    g, _, _ = _case()
    valid = np.ones(SHAPE, bool)
    valid[8, 9, 10] = False
    full = pkg.mesh.marching_cubes(_t(g, dev), LEVEL, LO, STEP)
    v, f, n = _run(pkg, dev, g, valid)
    cells = np.stack(np.unravel_index(RC.face_cells(g, LEVEL), [s - 1 for s in SHAPE]), 1)
    hit = np.all((cells >= (7, 8, 9)) & (cells <= (8, 9, 10)), axis=1)
    assert hit.sum() > 0 and len(f) == len(full[1]) - int(hit.sum())
    m = pkg.mesh.filter_faces(pkg.mesh.Mesh(*full, None), _t(~hit, dev))
    assert _same(v, m.verts) and _same(f, m.faces) and _same(n, m.normals)
    want = RC.marching_cubes_masked(g, valid, LEVEL, LO, STEP)
    assert _bits(v, want[0]) and _bits(f, want[1])


def test_capacities_one_row_short_clamp(pkg, dev):
    g, valid, want = _case()
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    s, m = _t(g, dev), _t(valid.astype(np.uint8), dev)
    V, F = len(want[0]), len(want[1])
    ws = torch.empty(pkg._abi.mesh_ws_bytes(*SHAPE), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lo, step = pkg._abi.f32_array(LO), pkg._abi.f32_array(STEP)
    GUARD = 64
    pkg._abi.check(L.nerf_hip_mesh_count_masked(s.data_ptr(), m.data_ptr(), *SHAPE, LEVEL, ws.data_ptr(), ws.numel(), counts.data_ptr(), st))
    verts = torch.full((V - 1 + GUARD, 3), 7.25, device=dev)
    normals = torch.full((V - 1 + GUARD, 3), -3.5, device=dev)
    faces = torch.full((F - 1 + GUARD, 3), -77, dtype=torch.int32, device=dev)
    pkg._abi.check(L.nerf_hip_mesh_emit_masked(s.data_ptr(), m.data_ptr(), *SHAPE, lo, step, LEVEL, ws.data_ptr(), ws.numel(), verts.data_ptr(),
                                               normals.data_ptr(), faces.data_ptr(), V - 1, F - 1, st))
    torch.cuda.synchronize()
    assert counts.tolist() == [V, F]
    assert (verts[V - 1:] == 7.25).all() and (normals[V - 1:] == -3.5).all() and (faces[F - 1:] == -77).all()
    assert _bits(verts[:V - 1], want[0][:V - 1]) and _bits(faces[:F - 1], want[1][:F - 1])


def test_host_refusals_launch_nothing(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    shape = (8, 8, 8)
    s = torch.rand(shape, device=dev)
    m = torch.ones(shape, dtype=torch.uint8, device=dev)
    ws = torch.empty(pkg._abi.mesh_ws_bytes(*shape), dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -5, dtype=torch.int64, device=dev)
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    out = torch.full((64, 3), 9.0, device=dev)
    fo = torch.full((64, 3), 9, dtype=torch.int32, device=dev)

    def rc_count(*dims, mp=m.data_ptr(), level=0.5, nbytes=ws.numel()):
        return L.nerf_hip_mesh_count_masked(s.data_ptr(), mp, *dims, level, ws.data_ptr(), nbytes, counts.data_ptr(), st)

    def rc_emit(*dims, mp=m.data_ptr(), level=0.5, stp=step, nbytes=ws.numel()):
        return L.nerf_hip_mesh_emit_masked(s.data_ptr(), mp, *dims, lo, stp, level, ws.data_ptr(), nbytes, out.data_ptr(), out.data_ptr(),
                                           fo.data_ptr(), 64, 64, st)

    assert rc_count(*shape, mp=None) == -1 and rc_emit(*shape, mp=None) == -1
    assert rc_count(*shape, nbytes=ws.numel() - 256) == -2 and rc_emit(*shape, nbytes=ws.numel() - 256) == -2
    assert rc_count(0, 8, 8) == -1 and rc_emit(8, 0, 8) == -1
    assert rc_count(*shape, level=float("nan")) == -1 and rc_emit(*shape, stp=pkg._abi.f32_array([1, -1, 1])) == -1
    torch.cuda.synchronize()
    assert (counts == -5).all() and (out == 9.0).all() and (fo == 9).all()
    assert rc_count(1, 8, 64) == 0  # a dimension of one point: the empty mesh
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
    # the Python layer
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.marching_cubes(s, 0.5, valid=m.cpu())
    with pytest.raises(ValueError, match="valid"):
        pkg.mesh.marching_cubes(s, 0.5, valid=m[:4])
    with pytest.raises(ValueError, match="valid"):
        pkg.mesh.marching_cubes(s, 0.5, valid=m.float())
