"""CPU: the point-query entry points (nerf_hip_query_ws_bytes / nerf_hip_query / nerf_hip_density_grid) are declared, bound and
exported, and refuse bad arguments before anything touches a device; the driver parses its density-grid options."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

QUERY_SYMBOLS = ("nerf_hip_query_ws_bytes", "nerf_hip_query", "nerf_hip_density_grid")


def test_abi_7_declared_bound_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    declared = set(re.findall(r"\b(nerf_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    for name in QUERY_SYMBOLS:
        assert name in declared and name in pkg._abi.EXPORTS and hasattr(lib, name), name
    assert pkg._abi.NERF_HIP_ABI_VERSION == 7
    assert pkg._abi.lib().nerf_hip_abi_version() == 7


def test_query_workspace_does_not_grow_with_points(pkg):
    n0, n1 = pkg._abi.query_ws_bytes(False), pkg._abi.query_ws_bytes(True)
    # packed weight image + fold, and for colour queries one fixed chunk of direction vectors: no argument that could carry M or a grid
    assert 0 < n0 < n1 < 256 << 20
    assert n0 % 256 == 0 and n1 % 256 == 0
    assert pkg._abi.query_ws_bytes(True) == n1


def _rc_text(pkg, rc):
    return rc, pkg._abi.lib().nerf_hip_last_error().decode()


def test_bad_grids_are_refused(pkg):
    L = pkg._abi.lib()
    lo, step = pkg._abi.f32_array([0, 0, 0]), pkg._abi.f32_array([1, 1, 1])
    # 2048 x 1024 x 1024 = 2^31 points: the kernels index points with 32-bit integers
    for dims in ((2048, 1024, 1024), (65536, 65536, 2)):
        with pytest.raises(pkg._abi.NerfHipError, match="2\\^31"):
            pkg._abi.check(L.nerf_hip_density_grid(None, lo, step, *dims, None, None, 0, None))
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        with pytest.raises(pkg._abi.NerfHipError, match="positive"):
            pkg._abi.check(L.nerf_hip_density_grid(None, lo, step, *dims, None, None, 0, None))
    rc, text = _rc_text(pkg, L.nerf_hip_density_grid(None, lo, step, 2048, 1024, 1024, None, None, 0, None))
    assert rc == -1 and text  # NERF_HIP_ERR_ARG with a message


def test_bad_queries_are_refused(pkg):
    L = pkg._abi.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    with pytest.raises(pkg._abi.NerfHipError, match="dirs and rgb"):
        pkg._abi.check(L.nerf_hip_query(None, p, None, 4, p, p, None, 0, None))  # rgb without dirs
    with pytest.raises(pkg._abi.NerfHipError, match="dirs and rgb"):
        pkg._abi.check(L.nerf_hip_query(None, p, p, 4, None, p, None, 0, None))  # dirs without rgb
    with pytest.raises(pkg._abi.NerfHipError, match="< 0"):
        pkg._abi.check(L.nerf_hip_query(None, p, None, -1, None, p, None, 0, None))
    assert L.nerf_hip_query(None, None, None, 0, None, None, None, 0, None) == 0  # M == 0: nothing to do, nothing launched
    # a workspace that is too small is refused before any launch (checked ahead of the device)
    w = (ctypes.c_void_p * 24)(*([1 << 20] * 24))  # (pointer values only: nothing is dereferenced before the refusal)
    rc, text = _rc_text(pkg, L.nerf_hip_query(w, p, None, 4, None, p, ctypes.c_void_p(1 << 20), 1024, None))
    assert rc == -2 and "workspace" in text


def test_cli_parses_density_grid_options(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    a = ap.parse_args(["--conf", "lego", "--density-grid", "128", "--grid-bbox", "-1", "-2", "-3", "1", "2", "3.5"])
    assert a.density_grid == 128 and a.grid_bbox == [-1.0, -2.0, -3.0, 1.0, 2.0, 3.5]
    d = ap.parse_args([])
    assert d.density_grid is None and d.grid_bbox == [-1.5] * 3 + [1.5] * 3
    with pytest.raises(SystemExit):
        ap.parse_args(["--grid-bbox", "1", "2", "3"])


def test_grid_step_is_fp32_on_the_host(pkg):
    from nerf_tiny_amd.nerf import grid_shape, grid_step

    assert grid_shape(5) == (5, 5, 5) and grid_shape((37, 20, 45)) == (37, 20, 45)
    lo, hi = np.float32([-1.5, -0.7, 0.1]), np.float32([1.5, 0.9, 0.1])
    st = grid_step(lo, hi, (37, 20, 1))
    assert st.dtype == np.float32
    assert st[0] == (np.float32(1.5) - np.float32(-1.5)) / np.float32(36)
    assert st[1] == (np.float32(0.9) - np.float32(-0.7)) / np.float32(19)
    assert st[2] == 0.0  # a single point along z
