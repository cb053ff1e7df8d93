"""CPU: nerf_hip_forward_maps (per-ray depth and opacity) is declared, bound and exported under ABI version 7, refuses training calls and a
null maps pointer before anything touches a device; the driver parses --maps; gather_rows keeps its shard checks for rows of width 4."""
import ctypes
import importlib
import os
import re

import pytest
import torch

from conftest import ROOT


def test_forward_maps_declared_bound_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr)
    assert re.search(r"\bnerf_hip_forward_maps\s*\(", hdr)
    assert "nerf_hip_forward_maps" in pkg._abi.EXPORTS
    assert hasattr(ctypes.CDLL(pkg._abi.LIB_PATH), "nerf_hip_forward_maps")
    # the arguments of nerf_hip_forward with `maps` behind C_fine
    fwd = pkg._abi._PROTOS["nerf_hip_forward"][1]
    assert pkg._abi._PROTOS["nerf_hip_forward_maps"][1] == fwd[:12] + [ctypes.c_void_p] + fwd[12:]
    assert pkg._abi.lib().nerf_hip_abi_version() == 7


def _call(pkg, flags, maps):
    L = pkg._abi.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    w = (ctypes.c_void_p * 24)(*([1 << 20] * 24))  # (pointer values only: nothing is dereferenced before the refusal)
    K9 = pkg._abi.f32_array([1, 0, 0, 0, 1, 0, 0, 0, 1])
    return L.nerf_hip_forward_maps(w, p, p, p, K9, None, 8, 64, 128, 1e-4, p, p, maps if maps is None else p, ctypes.c_void_p(1 << 20),
                                   1 << 30, flags, None)


def test_forward_maps_refuses_training_calls_and_null_maps(pkg):
    for flags in (pkg._abi.SAVE_FOR_BACKWARD, pkg._abi.SAVE_FOR_BACKWARD | pkg._abi.BF16_MLP):
        with pytest.raises(pkg._abi.NerfHipError, match="inference only"):
            pkg._abi.check(_call(pkg, flags, True))
    for flags in (0, pkg._abi.BF16_MLP, pkg._abi.SPLIT_MLP, pkg._abi.CORRECTED):
        with pytest.raises(pkg._abi.NerfHipError, match="maps is null"):
            pkg._abi.check(_call(pkg, flags, None))
    assert _call(pkg, 0, None) == -1  # NERF_HIP_ERR_ARG


def test_cli_parses_maps(pkg):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    assert ap.parse_args(["--maps"]).maps is True
    assert ap.parse_args([]).maps is False
    assert "display(maps=args.maps)" in open(os.path.join(ROOT, "nerf-tiny_amd", "main.py")).read()


def test_gather_rows_keeps_its_shard_checks_at_width_4(pkg):
    par = pkg.parallel
    n = 1003
    full = torch.arange(n * 4, dtype=torch.float32).view(n, 4)
    assert torch.equal(par.gather_rows(full.clone(), n, 0, 1), full)
    assert torch.equal(par.gather_rows(full.clone(), n, 0, 1, batch=100), full)
    with pytest.raises(ValueError, match="holds 1002 rows"):
        par.gather_rows(full[:-1].clone(), n, 0, 1)
    with pytest.raises(ValueError, match="holds 600 rows"):
        par.gather_rows(full[:600].clone(), n, 1, 2, batch=100)  # rank 1's shard on the batch grid is [600, 1003)
    with pytest.raises(ValueError, match="not both"):
        par.gather_rows(full.clone(), n, 0, 1, bounds=[(0, n)], batch=100)
    # a rank with an empty shard (more ranks than batches) hands over [0, 4]
    assert par.batch_shard_bounds(150, 100, 2, 3) == (150, 150)
    with pytest.raises(ValueError, match="holds 1 rows"):
        par.gather_rows(torch.zeros(1, 4), 150, 2, 3, batch=100)
