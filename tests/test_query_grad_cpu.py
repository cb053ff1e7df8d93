"""CPU: the gradient-query entry points (nerf_hip_query_grad_ws_bytes / nerf_hip_query_grad) are declared, bound and exported, their
workspace does not grow with the point count, every bad argument is refused before anything touches a device, and the driver parses
--mesh-normals."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import ROOT

GRAD_SYMBOLS = ("nerf_hip_query_grad_ws_bytes", "nerf_hip_query_grad")
CHUNK = 256 * 4 * 32 * 4  # points per chunk (kernels.h QGRAD_CHUNK): 4 rounds of one wave per SIMD


def test_declared_bound_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    declared = set(re.findall(r"\b(nerf_hip_[a-z_0-9]+)\s*\(", hdr))
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    for name in GRAD_SYMBOLS:
        assert name in declared and name in pkg._abi.EXPORTS and hasattr(lib, name), name


def test_workspace_is_independent_of_points_and_within_budget(pkg):
    n0, n1 = pkg._abi.query_grad_ws_bytes(False), pkg._abi.query_grad_ws_bytes(True)
    assert n0 % 256 == 0 and n1 % 256 == 0 and 0 < n0 < n1
    assert pkg._abi.query_grad_ws_bytes(True) == n1 and pkg._abi.query_grad_ws_bytes(False) == n0  # no argument could carry M
    # the per-point budget x the chunk (weight image included): 1.5 KB sigma only, 2.5 KB with colour -- the 10 KB training save is not
    # what is kept; and at least the masks + gamma_p rows (512 B), + c rows and direction vectors (1 KB more) of a whole chunk
    assert 512 * CHUNK <= n0 <= 1536 * CHUNK
    assert 1536 * CHUNK <= n1 <= 2560 * CHUNK


def _err(pkg, rc):
    return rc, pkg._abi.lib().nerf_hip_last_error().decode()


def test_bad_arguments_are_refused(pkg):
    L = pkg._abi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = None
    # (weights, points, dirs, M, dsigma, drgb, rgb, sigma, dpoints, ws, ws_bytes, stream)
    with pytest.raises(pkg._abi.NerfHipError, match="< 0"):
        pkg._abi.check(L.nerf_hip_query_grad(n, p, n, -1, n, n, n, p, p, n, 0, n))
    for pts, sig, dpts in ((n, p, p), (p, n, p), (p, p, n)):  # points, sigma, dpoints are required
        with pytest.raises(pkg._abi.NerfHipError, match="null argument"):
            pkg._abi.check(L.nerf_hip_query_grad(n, pts, n, 4, n, n, n, sig, dpts, n, 0, n))
    with pytest.raises(pkg._abi.NerfHipError, match="drgb needs dirs"):
        pkg._abi.check(L.nerf_hip_query_grad(n, p, n, 4, n, p, n, p, p, n, 0, n))
    with pytest.raises(pkg._abi.NerfHipError, match="dirs and rgb"):
        pkg._abi.check(L.nerf_hip_query_grad(n, p, p, 4, n, n, n, p, p, n, 0, n))  # dirs without rgb
    with pytest.raises(pkg._abi.NerfHipError, match="dirs and rgb"):
        pkg._abi.check(L.nerf_hip_query_grad(n, p, n, 4, n, n, p, p, p, n, 0, n))  # rgb without dirs
    # M == 0: nothing to do, nothing launched (and no weights or workspace needed)
    assert L.nerf_hip_query_grad(n, p, n, 0, n, n, n, p, p, n, 0, n) == 0
    # workspace refusals come ahead of the device check (pointer values only: nothing is dereferenced before the refusal)
    w = (ctypes.c_void_p * 24)(*([1 << 20] * 24))
    need0, need1 = pkg._abi.query_grad_ws_bytes(False), pkg._abi.query_grad_ws_bytes(True)
    rc, text = _err(pkg, L.nerf_hip_query_grad(w, p, n, 4, n, n, n, p, p, ctypes.c_void_p(1 << 20), need0 - 256, n))
    assert rc == -2 and "workspace" in text
    rc, text = _err(pkg, L.nerf_hip_query_grad(w, p, p, 4, n, p, p, p, p, ctypes.c_void_p(1 << 20), need1 - 256, n))
    assert rc == -2 and "workspace" in text
    rc, text = _err(pkg, L.nerf_hip_query_grad(w, p, n, 4, n, n, n, p, p, ctypes.c_void_p((1 << 20) + 128), need0, n))
    assert rc == -1 and "256-byte" in text
    rc, text = _err(pkg, L.nerf_hip_query_grad(w, p, n, 4, n, n, n, p, p, n, need0, n))
    assert rc == -1 and "workspace" in text


def test_cli_parses_mesh_normals(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    assert ap.parse_args([]).mesh_normals == "grid"
    assert ap.parse_args(["--mesh", "64", "--mesh-normals", "field"]).mesh_normals == "field"
    assert ap.parse_args(["--mesh-normals", "grid"]).mesh_normals == "grid"
    with pytest.raises(SystemExit):
        ap.parse_args(["--mesh-normals", "sobel"])


def test_extract_mesh_refuses_unknown_normals(pkg, oracle):
    m = pkg.NeRFModel(64, 128, 8)
    with pytest.raises(ValueError, match="normals"):
        m.extract_mesh((-1,) * 3, (1,) * 3, 4, 0.5, normals="sobel")
