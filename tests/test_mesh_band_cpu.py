"""CPU: the narrow-band grid's numpy restatement (tests/band_reference.py) gives the dense mesh bit for bit on the analytic blob, with
the evaluated-point counts computed when the feature was designed; an island smaller than a block is missed (the documented limit); the
blob MLP is the analytic field through the oracle; header, binding and library carry the band calls under ABI 7; the calls refuse bad
arguments before any device work; the driver parses --mesh-band."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import band_reference as B
import mc_reference as R
from conftest import ROOT

BAND_SYMBOLS = ("nerf_hip_band_ws_bytes", "nerf_hip_band_begin", "nerf_hip_band_grow")
TABLE = R.load_table()


def _same_mesh(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("shape,r,thr,V,F,trace", [c for c in B.CASES if np.prod(c[0]) <= 65 ** 3], ids=lambda v: None)
def test_band_gives_the_dense_mesh_on_the_blob(shape, r, thr, V, F, trace):
    dense = B.blob_analytic(shape, thr)
    out, info = B.band(dense, B.LEVEL, r)
    _, step = B.blob_points(shape)
    want = R.marching_cubes(dense, B.LEVEL, B.BOX_LO, step, TABLE)
    got = R.marching_cubes(out, B.LEVEL, B.BOX_LO, step, TABLE)
    assert (len(want[0]), len(want[1])) == (V, F)
    assert _same_mesh(want, got)
    assert info["trace"] == trace and info["rounds"] == len(trace)
    nb = [-(-n // r) for n in shape]
    assert info["blocks_total"] == int(np.prod(nb)) and info["blocks_active"] == sum(t[0] for t in trace)
    assert info["points_total"] == int(np.prod(shape)) and info["points_evaluated"] < 0.5 * info["points_total"]
    # evaluated points keep the dense bits; the others hold a value of their own class wherever a cell is mixed
    closed, chi, vol, _ = R.mesh_stats(got[0], got[1])
    assert closed and chi == 2 and vol > 0


def test_band_on_a_random_grid_activates_everything():
    dense = np.random.default_rng(11).random((33, 29, 37), dtype=np.float32)
    out, info = B.band(dense, 0.5, 4)
    assert info["blocks_active"] == info["blocks_total"] == 9 * 8 * 10
    assert np.array_equal(out, dense)
    # every block once, plus the unique corner points of the first pass
    assert info["points_evaluated"] == dense.size + 9 * 8 * 10
    assert _same_mesh(R.marching_cubes(dense, 0.5, table=TABLE), R.marching_cubes(out, 0.5, table=TABLE))


def test_counting_rules():
    # corner planes: unique min(b r, n - 1)
    assert B.corner_indices(49, 4).tolist() == list(range(0, 49, 4))
    assert B.corner_indices(50, 4).tolist() == list(range(0, 49, 4)) + [49]
    assert B.corner_indices(1, 4).tolist() == [0] and B.corner_indices(3, 8).tolist() == [0, 2]
    # nothing / everything inside: no seeds, only the corner pass
    dense = B.blob_analytic((49, 49, 49), 1.5)
    for level in (200.0, -1.0):
        out, info = B.band(dense, level, 4)
        assert info["rounds"] == 0 and info["blocks_active"] == 0 and info["points_evaluated"] == 13 ** 3
        assert len(R.marching_cubes(out, level, table=TABLE)[0]) == 0
    with pytest.raises(ValueError):
        B.band(dense, 30.0, 1)


def test_an_island_smaller_than_a_block_is_missed():
    """The documented limit: a component that fits between the corner samples is invisible."""
    dense = B.blob_analytic((65, 65, 65), 1.5)
    dense[3:6, 3:6, 3:6] = 100.0  # far from the blob, strictly inside block (0, 0, 0) of 8^3
    out, info = B.band(dense, B.LEVEL, 8)
    want = R.marching_cubes(dense, B.LEVEL, table=TABLE)
    got = R.marching_cubes(out, B.LEVEL, table=TABLE)
    assert (len(want[0]), len(got[0])) == (5748, 5694)
    # with blocks the island cannot hide in, it is found
    out2, _ = B.band(dense, B.LEVEL, 2)
    assert _same_mesh(want, R.marching_cubes(out2, B.LEVEL, table=TABLE))
    # a whole object inside one block: the empty mesh
    out3, info3 = B.band(B.blob_analytic((40, 40, 40), 2.2), B.LEVEL, 64)
    assert info3["rounds"] == 0 and info3["blocks_total"] == 1 and len(R.marching_cubes(out3, B.LEVEL, table=TABLE)[0]) == 0


def test_blob_mlp_is_the_analytic_field(oracle):
    import torch

    shape, thr = (33, 33, 33), 2.4  # a row of the table: every lattice point of it
    axes, _ = B.blob_points(shape)
    pts = torch.from_numpy(np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(1, -1, 3))
    fp, fd = oracle.frequencies()
    assert float(fp[0]) == float(np.float32(np.pi))
    gp = oracle.encode(pts, fp)
    gd = oracle.encode(torch.zeros_like(pts), fd)
    sigma = oracle.mlp(B.blob_weights(oracle, thr), gp, gd)[1].numpy()[0]
    want = 100 * np.maximum(0, np.cos(np.pi * pts.double().numpy()[0]).sum(1) - thr)
    assert (want > B.LEVEL).sum() > 20
    assert np.abs(sigma - want).max() < 7e-5
    assert np.abs(B.blob_analytic(shape, thr).reshape(-1) - want).max() < 7e-5


def test_band_abi_declared_bound_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    assert pkg._abi.NERF_HIP_ABI_VERSION == 7
    declared = set(re.findall(r"\b(nerf_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    assert lib.nerf_hip_abi_version() == 7
    for name in BAND_SYMBOLS:
        assert name in declared and name in pkg._abi.EXPORTS and hasattr(lib, name), name


def test_band_ws_bytes(pkg):
    w = pkg._abi.band_ws_bytes
    q = pkg._abi.query_ws_bytes(False)
    n = w(512, 512, 512, 8)
    assert n % 256 == 0 and q + 10 * 64 ** 3 <= n < q + 11 * 64 ** 3  # 10 bytes per block, nothing per lattice point
    assert w(512, 512, 512, 4) > n > w(512, 512, 512, 16)
    assert w(40, 40, 40, 64) == w(40, 40, 40, 1 << 30)  # a block beyond the grid is one block
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        with pytest.raises(pkg._abi.NerfHipError, match="positive"):
            w(*dims, 8)
    with pytest.raises(pkg._abi.NerfHipError, match="2\\^31"):
        w(2048, 1024, 1024, 8)
    for block in (1, 0, -3):
        with pytest.raises(pkg._abi.NerfHipError, match="block"):
            w(64, 64, 64, block)
    with pytest.raises(pkg._abi.NerfHipError, match="blocks"):
        w(1024, 1024, 1024, 2)


def test_band_calls_refuse_bad_arguments(pkg):
    L = pkg._abi.lib()
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = ctypes.c_void_p(1 << 20)  # (pointer values only: nothing is dereferenced before a refusal)
    w24 = (ctypes.c_void_p * 24)(*[p.value] * 24)

    def begin(*dims, block=4, level=0.5, ws_=ws, ws_bytes=1 << 30, sigma=p, counts=p, lo_=lo, w=w24):
        return pkg._abi.check(L.nerf_hip_band_begin(w, lo_, step, *dims, block, level, sigma, ws_, ws_bytes, counts, None))

    def grow(*dims, block=4, level=0.5, ws_=ws, ws_bytes=1 << 30, sigma=p, counts=p, lo_=lo, w=w24, n=1):
        return pkg._abi.check(L.nerf_hip_band_grow(w, lo_, step, *dims, block, level, n, sigma, ws_, ws_bytes, counts, None))

    for call in (begin, grow):
        for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            with pytest.raises(pkg._abi.NerfHipError, match="positive"):
                call(*dims)
        for dims in ((2048, 1024, 1024), (65536, 65536, 2)):
            with pytest.raises(pkg._abi.NerfHipError, match="2\\^31"):
                call(*dims)
        for block in (1, 0, -2):
            with pytest.raises(pkg._abi.NerfHipError, match="block"):
                call(8, 8, 8, block=block)
        for lv in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(pkg._abi.NerfHipError, match="not finite"):
                call(8, 8, 8, level=lv)
        with pytest.raises(pkg._abi.NerfHipError, match="sigma is null"):
            call(8, 8, 8, sigma=None)
        with pytest.raises(pkg._abi.NerfHipError, match="lo3"):
            call(8, 8, 8, lo_=None)
        with pytest.raises(pkg._abi.NerfHipError, match="workspace is null"):
            call(8, 8, 8, ws_=None)
        with pytest.raises(pkg._abi.NerfHipError, match="aligned"):
            call(8, 8, 8, ws_=ctypes.c_void_p((1 << 20) + 64))
        with pytest.raises(pkg._abi.NerfHipError, match="error -2: workspace"):
            call(8, 8, 8, ws_bytes=pkg._abi.band_ws_bytes(8, 8, 8, 4) - 1)
        with pytest.raises(pkg._abi.NerfHipError, match="counts"):
            call(8, 8, 8, counts=None)
        with pytest.raises(pkg._abi.NerfHipError, match="8-byte"):
            call(8, 8, 8, counts=ctypes.c_void_p(p.value + 4))
        with pytest.raises(pkg._abi.NerfHipError):  # a null weight table / pointer
            call(8, 8, 8, w=None)
    for n in (-1, 9):  # the 8^3 grid has 8 blocks of 4^3
        with pytest.raises(pkg._abi.NerfHipError, match="n_blocks"):
            grow(8, 8, 8, n=n)
    # the mesh calls' error codes: -1 arguments, -2 workspace
    assert L.nerf_hip_band_grow(w24, lo, step, 8, 8, 8, 1, 0.5, 0, p, ws, 1 << 30, p, None) == -1
    assert L.nerf_hip_band_grow(w24, lo, step, 8, 8, 8, 4, 0.5, 0, p, ws, 16, p, None) == -2


def test_band_needs_a_device_model(pkg, oracle):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.density_band((-1,) * 3, (1,) * 3, 16, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.extract_mesh((-1,) * 3, (1,) * 3, 16, 0.5, band=4)


def test_cli_parses_mesh_band(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    a = ap.parse_args(["--mesh", "256", "--mesh-band", "8"])
    assert a.mesh == 256 and a.mesh_band == 8
    assert ap.parse_args(["--mesh", "64"]).mesh_band is None
