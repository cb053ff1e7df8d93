"""GPU: the narrow-band density grid (nerf_hip_band_begin / nerf_hip_band_grow, ops.density_band, NeRFModel.density_band,
extract_mesh(band=r)) against the numpy restatement in tests/band_reference.py run on the device's OWN dense grid -- arrays and counts
bit for bit -- and the banded mesh against the dense mesh of the same call; degenerate grids; refusals; stores that stay inside the
caller's buffers."""
import glob

import numpy as np
import pytest
import torch

import band_reference as B
import mc_reference as R
from test_mesh_cpu import _read_ply

pytestmark = pytest.mark.gpu

INFO = ("rounds", "blocks_active", "blocks_total", "points_evaluated", "points_total")
_models = {}


def _blob(pkg, oracle, dev, thr):
    if thr not in _models:
        m = pkg.NeRFModel(64, 128, 8)
        m.load_state_dict(B.blob_weights(oracle, thr))
        _models[thr] = m.to(dev)
    return _models[thr]


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    return np.ascontiguousarray(a).view(np.int32)


def _check_against_restatement(m, lo, hi, shape, level, r):
    dense = m.density_grid(lo, hi, shape).cpu().numpy()
    want, winfo = B.band(dense, level, r)
    sigma, info = m.density_band(lo, hi, shape, level, block=r)
    assert sigma.dtype == torch.float32 and tuple(sigma.shape) == tuple(shape) and sigma.is_cuda
    print(f"band {shape} r={r}: device {info}, restatement trace {winfo['trace']}")
    assert set(info) == set(INFO)
    assert {k: winfo[k] for k in INFO} == info
    assert np.array_equal(_bits(sigma), _bits(want))
    return sigma, winfo


@pytest.mark.parametrize("shape,r,thr,V,F,trace", B.CASES, ids=lambda v: None)
def test_band_matches_the_restatement_and_the_dense_mesh(oracle, pkg, dev, shape, r, thr, V, F, trace):
    m = _blob(pkg, oracle, dev, thr)
    _, winfo = _check_against_restatement(m, B.BOX_LO, B.BOX_HI, shape, B.LEVEL, r)
    # conditions on the restatement's own numbers, so that the comparison above cannot go hollow
    if len(trace) >= 2:
        assert winfo["rounds"] >= 2
    assert winfo["rounds"] >= 1 and winfo["points_evaluated"] < 0.5 * winfo["points_total"]
    dense = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL)
    band = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, band=r)
    assert len(dense.verts) > 200 and len(dense.faces) > 400
    for a, b in zip(band, dense):
        assert torch.equal(a, b)
    if shape == (50, 41, 45):
        fd = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, normals="field")
        fb = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, normals="field", band=r)
        assert not torch.equal(fd.normals, dense.normals)
        for a, b in zip(fb, fd):
            assert torch.equal(a, b)


def test_block_scan_with_more_totals_than_scan_threads(oracle, pkg, dev):
    """130 x 128 x 128 in blocks of 2: 65 * 64 * 64 = 266,240 blocks, 1,040 workgroup totals -- the scan's threads take runs of two, in
    the int channel (new blocks, with bases) and in the 64-bit one (their points, the total only)."""
    shape, r = (130, 128, 128), 2
    assert -(-(65 * 64 * 64) // 256) > 1024
    m = _blob(pkg, oracle, dev, 1.5)
    _, winfo = _check_against_restatement(m, B.BOX_LO, B.BOX_HI, shape, B.LEVEL, r)
    assert winfo["rounds"] >= 1 and winfo["blocks_total"] == 266240 and winfo["blocks_active"] > 2048
    dense = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL)
    band = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, band=r)
    assert len(dense.faces) > 10000
    for a, b in zip(band, dense):
        assert torch.equal(a, b)


def test_rough_field_is_the_composition(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, True))
    m = m.to(dev)
    lo, hi, shape = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), (37, 20, 45)
    level = float(m.density_grid(lo, hi, shape).median())
    sigma, _ = _check_against_restatement(m, lo, hi, shape, level, 4)
    from nerf_tiny_amd.nerf import grid_step

    step = grid_step(np.float32(lo), np.float32(hi), shape)
    v, f, n = pkg.mesh.marching_cubes(sigma, level, lo, step)
    out = m.extract_mesh(lo, hi, shape, level, band=4)
    assert len(out.faces) > 100
    for a, b in zip(out, (v, f, n, m.query(v, -n)[0])):
        assert torch.equal(a, b)
    rv, rf, _ = R.marching_cubes(sigma.cpu().numpy(), level, lo, step)
    assert np.array_equal(_bits(out.verts), _bits(rv)) and np.array_equal(out.faces.cpu().numpy(), rf)


def test_degenerate_grids(oracle, pkg, dev):
    m = _blob(pkg, oracle, dev, 1.5)
    shape = (49, 49, 49)
    for level in (200.0, -1.0):  # nothing / everything inside: no seeds
        _, winfo = _check_against_restatement(m, B.BOX_LO, B.BOX_HI, shape, level, 4)
        assert winfo["rounds"] == 0 and winfo["blocks_active"] == 0 and winfo["points_evaluated"] == 13 ** 3
        out = m.extract_mesh(B.BOX_LO, B.BOX_HI, shape, level, band=4)
        assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3)
    # one point along z (the slice z = 0 through the blob): blocks, seeds and a round, but no cells
    slo, shi = (-1.0, -1.0, 0.0), (1.0, 1.0, 0.0)
    _, winfo = _check_against_restatement(m, slo, shi, (49, 49, 1), B.LEVEL, 4)
    assert winfo["rounds"] >= 1
    assert m.extract_mesh(slo, shi, (49, 49, 1), B.LEVEL, band=4).faces.shape == (0, 3)
    # one point in all: a single block and a single corner
    _, winfo = _check_against_restatement(m, B.BOX_LO, B.BOX_LO, (1, 1, 1), B.LEVEL, 8)
    assert winfo["points_evaluated"] == 1 and winfo["blocks_total"] == 1
    # a block larger than the grid: one block whose corners are the grid's, all outside -- the blob is missed, nothing faults
    for r in (64, 1 << 30):
        _, winfo = _check_against_restatement(m, B.BOX_LO, B.BOX_HI, (40, 40, 40), B.LEVEL, r)
        assert winfo["blocks_total"] == 1 and winfo["rounds"] == 0 and winfo["points_evaluated"] == 8
    assert m.extract_mesh(B.BOX_LO, B.BOX_HI, (40, 40, 40), B.LEVEL, band=64).verts.shape == (0, 3)
    assert len(m.extract_mesh(B.BOX_LO, B.BOX_HI, (40, 40, 40), B.LEVEL).verts) > 0
    # ... and with one corner inside, that single block is evaluated whole
    sigma, winfo = _check_against_restatement(m, (0.0, 0.0, 0.0), B.BOX_HI, (21, 20, 19), B.LEVEL, 32)
    assert winfo["rounds"] == 1 and winfo["blocks_active"] == 1 and winfo["points_evaluated"] == 8 + 21 * 20 * 19


def test_refusals(oracle, pkg, dev):
    m = _blob(pkg, oracle, dev, 1.5)
    for block in (1, 0, -4):
        with pytest.raises(pkg._abi.NerfHipError, match="block"):
            m.density_band(B.BOX_LO, B.BOX_HI, 16, B.LEVEL, block=block)
        with pytest.raises(pkg._abi.NerfHipError, match="block"):
            m.extract_mesh(B.BOX_LO, B.BOX_HI, 16, B.LEVEL, band=block)
    for level in (float("nan"), float("inf")):
        with pytest.raises(pkg._abi.NerfHipError, match="not finite"):
            m.density_band(B.BOX_LO, B.BOX_HI, 16, level)
    with pytest.raises(pkg._abi.NerfHipError, match="positive"):
        m.density_band(B.BOX_LO, B.BOX_HI, (16, 0, 16), B.LEVEL)


def test_calls_stay_inside_their_buffers_and_refusals_launch_nothing(oracle, pkg, dev):
    m = _blob(pkg, oracle, dev, 1.5)
    ps = m._params()
    shape, r = (50, 41, 45), 4  # ragged along every axis
    N, GUARD = int(np.prod(shape)), 4096
    from nerf_tiny_amd.nerf import grid_step

    lo = np.float32(B.BOX_LO)
    step = grid_step(lo, np.float32(B.BOX_HI), shape)
    want, winfo = B.band(m.density_grid(B.BOX_LO, B.BOX_HI, shape).cpu().numpy(), B.LEVEL, r)
    big = torch.full((GUARD + N + GUARD,), -7.25, device=dev)
    cbig = torch.full((512 + 2 + 512,), -99, dtype=torch.int64, device=dev)
    nws = pkg._abi.band_ws_bytes(*shape, r)
    wbig = torch.full((nws + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    sigma, counts = big[GUARD:GUARD + N].view(*shape), cbig[512:514]
    # refused calls first: nothing may be written
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    head = (pkg._abi.ptr_array(ps), pkg._abi.f32_array(lo.tolist()), pkg._abi.f32_array(step.tolist()))
    tail = (sigma.data_ptr(), wbig.data_ptr())
    assert L.nerf_hip_band_begin(*head, *shape, r, B.LEVEL, *tail, nws - 256, counts.data_ptr(), st) == -2
    assert L.nerf_hip_band_grow(*head, *shape, r, B.LEVEL, 1, *tail, nws - 256, counts.data_ptr(), st) == -2
    assert L.nerf_hip_band_begin(*head, *shape, 1, B.LEVEL, *tail, nws, counts.data_ptr(), st) == -1
    assert L.nerf_hip_band_begin(*head, *shape, r, float("nan"), *tail, nws, counts.data_ptr(), st) == -1
    assert L.nerf_hip_band_begin(*head, 50, 0, 45, r, B.LEVEL, *tail, nws, counts.data_ptr(), st) == -1
    assert L.nerf_hip_band_grow(*head, *shape, r, B.LEVEL, -1, *tail, nws, counts.data_ptr(), st) == -1
    assert L.nerf_hip_band_begin(*head, *shape, r, B.LEVEL, *tail, nws, None, st) == -1
    torch.cuda.synchronize()
    assert (big == -7.25).all() and (cbig == -99).all() and (wbig == 0x5A).all()
    out, info = pkg.ops.density_band(ps, lo.tolist(), step.tolist(), shape, B.LEVEL, r, ws=wbig[:nws], sigma=sigma, counts=counts)
    torch.cuda.synchronize()
    assert out.data_ptr() == sigma.data_ptr() and {k: winfo[k] for k in INFO} == info
    assert np.array_equal(_bits(sigma), _bits(want))
    assert (big[:GUARD] == -7.25).all() and (big[GUARD + N:] == -7.25).all()
    assert (cbig[:512] == -99).all() and (cbig[514:] == -99).all() and counts.tolist() == [0, 0]
    assert (wbig[nws:] == 0x5A).all()


def test_other_weights_are_not_served_from_a_stale_image(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(B.blob_weights(oracle, 1.5))
    m = m.to(dev)
    shape, r = (49, 49, 49), 4
    a, ia = m.density_band(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, block=r)
    m.load_state_dict(B.blob_weights(oracle, 2.2))
    b, ib = _check_against_restatement(m, B.BOX_LO, B.BOX_HI, shape, B.LEVEL, r)
    assert ia["blocks_active"] > ib["blocks_active"] > 0 and not torch.equal(a, b)
    # in place, as an optimiser changes them
    with torch.no_grad():
        m.network.point_layer[7][0].bias[0] = -100.0 * (3.0 + 1.5)
    c, ic = m.density_band(B.BOX_LO, B.BOX_HI, shape, B.LEVEL, block=r)
    assert ic == ia and torch.equal(c, a)


def test_runner_exports_a_banded_mesh(pkg, dev, tmp_path):
    scene = pkg.data.synthetic_scene(n_pic=4, H=32, W=32, seed=1)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=6, batch_ray=256, learning=3e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1000, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1000)
    run = pkg.NeRFRunner(continue_=False, **kw)
    assert run.trainer("train") == 5
    level = float(np.median(run.density_grid(32, save=False)))
    out = run.extract_mesh(32, level, save=True, band=4)
    files = glob.glob(rs + "*_5_mesh32.ply")
    assert len(files) == 1
    want = run.model.extract_mesh((-1.5,) * 3, (1.5,) * 3, 32, level, band=4)
    assert len(out.faces) > 0
    for a, b in zip(out, want):
        assert np.array_equal(a, b.cpu().numpy())
    _, V, F = _read_ply(files[0])
    assert np.array_equal(np.stack([V["x"], V["y"], V["z"]], 1), out.verts) and np.array_equal(F["i"], out.faces)
    run.rank = 1  # under a launcher only rank 0 computes and writes
    assert run.extract_mesh(32, level, save=True, band=4) is None
    assert len(glob.glob(rs + "*_mesh32.ply")) == 1
