"""CPU: rule DL (include/nerf_hip.h) -- the distortion loss of one pass of a ray -- as tests/distortion_reference.py
restates it, and the interface the feature adds.

  1. the prefix form equals the O(N^2) definition in float64, on R.operands and R.tie_operands; their gradients agree where the m are
     distinct; the written-out dL/dw, dL/dt of the rule equal autograd of the prefix form (ties included: the index fixes the sign);
  2. properties: L = 0 for a ray whose weight is one sample with d = 0; L is invariant under t -> c t + b of t, near and far together; L >= 0;
  3. the interface: the six entries are declared, bound (argument counts as the header's) and exported; the two whole calls refuse what they
     must before any device work; distortion_loss on CPU tensors; forward(distortion=True)'s two ValueErrors; NeRFRunner(dist_weight=) refuses
     -1 / inf / nan before any device use; the driver parses --dist-weight and reads DIST_WEIGHT from an ini.
"""
import ctypes
import importlib
import inspect
import os
import re
from configparser import ConfigParser

import pytest
import torch

import distortion_reference as DR
import ray_stage_reference as R
from conftest import ROOT

F64 = torch.float64
SIZES = [(2, 1), (5, 3), (31, 65), (64, 128), (130, 200)]  # N = 3 .. 330 (the O(N^2) form at (1024, 1024) is 6 x 2048^2 doubles: left out)


def _passes(Nc, Nf):
    """float64 (t, w, near, far) of the coarse pass and of a merged, sorted pass built from R.operands (fine depths drawn inside the ray)"""
    o = R.operands(Nc, Nf)
    near, far = o["near"].double(), o["far"].double()
    delta_c = ((far - near) / Nc)[:, None].expand(-1, Nc)
    yield o["t_c"].double(), R.weights(delta_c, o["sig_c"].double()), near, far
    gen = torch.Generator().manual_seed(1)
    t_f = near[:, None] + (far - near)[:, None] * torch.rand(R.B_RAYS, Nf, generator=gen, dtype=F64)
    t_s = torch.sort(torch.cat((o["t_c"].double(), t_f), 1), dim=1).values
    sig = torch.cat((o["sig_c"], o["sig_f"]), 1).double()
    yield t_s, R.merged_composite(t_s, torch.zeros(R.B_RAYS, Nc + Nf, 3, dtype=F64), sig)["w"], near, far


def _tie_pass():
    o = R.tie_operands()
    t_s = torch.sort(torch.cat((o["t_c"], o["t_f"]), 1).double(), dim=1).values
    sig = torch.cat((o["sig_c"], o["sig_f"]), 1).double()
    B, N = t_s.shape
    assert int((t_s[:, 1:] == t_s[:, :-1]).sum()) > B  # exact duplicate depths, and with them duplicate midpoints
    return t_s, R.merged_composite(t_s, torch.zeros(B, N, 3, dtype=F64), sig)["w"], torch.full((B,), 1.5, dtype=F64), torch.full((B,), 6.5, dtype=F64)


def _autograd(fn, t, w, near, far):
    t, w = t.clone().requires_grad_(True), w.clone().requires_grad_(True)
    fn(t, w, near, far).sum().backward()
    return w.grad, t.grad


def _close(a, b, tol):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- 1 ----
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_prefix_form_is_the_pair_definition(Nc, Nf):
    for t, w, near, far in _passes(Nc, Nf):
        _close(DR.distortion(t, w, near, far), DR.distortion_pairs(t, w, near, far), 1e-12)
        m, _ = DR.midpoints(t)
        assert bool((m[:, 1:] > m[:, :-1]).all())  # distinct midpoints: the two forms have the same gradient
        for a, b in zip(_autograd(DR.distortion, t, w, near, far), _autograd(DR.distortion_pairs, t, w, near, far)):
            _close(a, b, 1e-12)
        for a, b in zip(DR.closed_form_grads(t, w, near, far), _autograd(DR.distortion, t, w, near, far)):
            _close(a, b, 1e-12)


def test_prefix_form_on_exact_ties():
    t, w, near, far = _tie_pass()
    _close(DR.distortion(t, w, near, far), DR.distortion_pairs(t, w, near, far), 1e-12)
    for a, b in zip(DR.closed_form_grads(t, w, near, far), _autograd(DR.distortion, t, w, near, far)):
        _close(a, b, 1e-12)  # (the pair form's |x| has subgradient 0 at a tie; the rule takes the sign of i - j: the prefix form's)


def test_one_and_two_sample_rays():
    near, far = torch.tensor([2.0], dtype=F64), torch.tensor([6.0], dtype=F64)
    t, w = torch.tensor([[3.0]], dtype=F64), torch.tensor([[0.7]], dtype=F64)
    assert float(DR.distortion(t, w, near, far)) == 0.0
    dw, dt = DR.closed_form_grads(t, w, near, far)
    assert float(dw) == 0.0 and float(dt) == 0.0
    t, w = torch.tensor([[3.0, 4.0]], dtype=F64), torch.tensor([[0.5, 0.25]], dtype=F64)
    # m = (3.5, 4), d = (1, 0): 2 w0 w1 (m1 - m0) + w0^2 / 3 = 0.125 + 0.25 / 3, over far - near = 4
    _close(DR.distortion(t, w, near, far), torch.tensor([(0.125 + 0.25 / 3) / 4], dtype=F64), 1e-15)
    for a, b in zip(DR.closed_form_grads(t, w, near, far), _autograd(DR.distortion, t, w, near, far)):
        _close(a, b, 1e-15)


# ---- 2 ----
def test_a_ray_with_its_weight_in_one_closed_sample_has_no_distortion():
    B, N = 3, 17
    t = torch.linspace(2, 6, N, dtype=F64).repeat(B, 1)
    near, far = torch.full((B,), 2.0, dtype=F64), torch.full((B,), 6.0, dtype=F64)
    w = torch.zeros(B, N, dtype=F64)
    w[:, -1] = 0.9  # the last sample: d = 0
    assert bool((DR.distortion(t, w, near, far) == 0).all()) and bool((DR.distortion_pairs(t, w, near, far) == 0).all())
    t[:, 5] = t[:, 4]  # a repeated depth closes the interval of sample 4
    w.zero_()
    w[:, 4] = 0.9
    assert bool((DR.distortion(t, w, near, far) == 0).all())


@pytest.mark.parametrize("Nc,Nf", [(5, 3), (64, 128)])
def test_invariant_under_affine_maps_of_depth_and_nonnegative(Nc, Nf):
    for t, w, near, far in _passes(Nc, Nf):
        L = DR.distortion(t, w, near, far)
        assert bool((L >= 0).all()) and bool((L > 0).any())
        for c, b in ((2.0, 0.0), (0.25, 3.0), (7.5, -11.0)):
            _close(DR.distortion(c * t + b, w, c * near + b, c * far + b), L, 1e-12)


# ---- 3 ----
NEW = {  # name -> (the entry it extends, the arguments it appends)
    "nerf_hip_forward_distortion_train": ("nerf_hip_forward_maps_train", 1),
    "nerf_hip_backward_distortion": ("nerf_hip_backward_maps", 1),
    "nerf_hip_coarse_composite_distortion": ("nerf_hip_coarse_composite_maps", 1),
    "nerf_hip_merge_composite_distortion": ("nerf_hip_merge_composite_train", 2),
    "nerf_hip_coarse_composite_backward_distortion": ("nerf_hip_coarse_composite_backward_maps", 1),
    "nerf_hip_merge_composite_backward_distortion": ("nerf_hip_merge_composite_backward", 2),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_hip.h")).read(), flags=re.S)


def _declared_args(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_distortion_entries_declared_bound_and_exported(pkg):
    hdr = _header()
    abi = pkg._abi
    so = ctypes.CDLL(abi.LIB_PATH)
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr) and abi.lib().nerf_hip_abi_version() == 7
    for name, (base, extra) in NEW.items():
        assert name in abi.EXPORTS and hasattr(so, name), name
        res, args = abi._PROTOS[name]
        assert res is ctypes.c_int
        assert len(args) == len(_declared_args(hdr, name)), name            # the binding has the header's argument count ...
        assert len(_declared_args(hdr, base)) == len(abi._PROTOS[base][1])  # ... as the entry it extends has
        assert args == abi._PROTOS[base][1] + [ctypes.c_void_p] * extra, name  # the base's arguments, then the new pointers
    raw = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert "DL. THE DISTORTION RULE" in raw and "QD. THE QUANTILE RULE" in raw


def _ptrs():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    w = (ctypes.c_void_p * 24)(*([1 << 20] * 24))  # (pointer values only: nothing is dereferenced before the refusal)
    return buf, p, w


def test_whole_calls_refuse_before_any_device_work(pkg):
    abi = pkg._abi
    L = abi.lib()
    buf, p, w = _ptrs()
    K9 = abi.f32_array([1, 0, 0, 0, 1, 0, 0, 0, 1])
    fwd = lambda flags, maps, dist: L.nerf_hip_forward_distortion_train(w, p, p, p, K9, None, 8, 64, 128, 1e-4, p, p, maps,
                                                                        ctypes.c_void_p(1 << 20), 1 << 30, flags, None, dist)
    S = abi.SAVE_FOR_BACKWARD
    for flags in (0, abi.BF16_MLP, abi.SPLIT_MLP, abi.CORRECTED, abi.FORCE_TILE_KERNEL):
        with pytest.raises(abi.NerfHipError, match="training only"):
            abi.check(fwd(flags, p, p))
    for flags in (S, S | abi.BF16_MLP, S | abi.SPLIT_MLP, S | abi.CORRECTED):
        for maps, dist in ((None, p), (p, None)):
            rc = fwd(flags, maps, dist)
            assert rc == -1  # NERF_HIP_ERR_ARG
            with pytest.raises(abi.NerfHipError, match="null"):
                abi.check(rc)
        for dmaps, ddist in ((None, p), (p, None)):
            rc = L.nerf_hip_backward_distortion(w, p, p, dmaps, None, 8, 64, 128, 1e-4, w, ctypes.c_void_p(1 << 20), 1 << 30, flags, None, None, ddist)
            assert rc == -1
            with pytest.raises(abi.NerfHipError, match="null"):
                abi.check(rc)


def test_distortion_loss_on_cpu_tensors(pkg):
    m = pkg.NeRFModel(64, 128, 4)
    dist = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0]], requires_grad=True)
    assert float(m.distortion_loss(dist).detach()) == 70.0
    total = m.distortion_loss(dist, coarse=True)
    assert float(total.detach()) == 77.0
    total.backward()
    assert torch.equal(dist.grad, torch.ones(3, 2))


def test_forward_refuses_distortion_without_maps_or_without_a_graph(pkg):
    m = pkg.NeRFModel(64, 128, 4)  # (a CPU model: both refusals come before the device is looked at)
    row = torch.zeros(4, dtype=torch.int64)
    pb, K = torch.zeros(4, 17), torch.eye(3)
    with pytest.raises(ValueError, match="maps=True"):
        m(row, row, pb, K, distortion=True)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"render\(quantiles=\)"):
            m(row, row, pb, K, maps=True, distortion=True)
    for p in m.network.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match=r"render\(quantiles=\)"):
        m(row, row, pb, K, maps=True, distortion=True)


def test_runner_refuses_a_bad_dist_weight_before_the_gpu(pkg):
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="dist_weight"):
            pkg.NeRFRunner(dist_weight=bad)
    assert inspect.signature(pkg.NeRFRunner.__init__).parameters["dist_weight"].default == 0.0
    train = importlib.import_module("nerf_tiny_amd.train")
    sig = inspect.signature(train.regularized_train_step)
    assert [sig.parameters[k].default for k in ("alpha", "mask_weight", "dist_weight")] == [None, 0.0, 0.0]


def test_cli_and_ini_parse_the_dist_weight(pkg, tmp_path):
    main = importlib.import_module("nerf_tiny_amd.main")
    ap = main.build_parser()
    assert ap.parse_args(["--dist-weight", "0.01"]).dist_weight == 0.01
    assert ap.parse_args([]).dist_weight is None  # -> the ini's DIST_WEIGHT, default 0
    ini = tmp_path / "x.ini"
    ini.write_text("[x]\nDIST_WEIGHT = 0.02\n[y]\nBATCH_RAY = 400\n")
    conf = ConfigParser()
    conf.read(str(ini))
    assert main.dist_weight_of(ap.parse_args(["--conf", "x"]), conf) == 0.02
    assert main.dist_weight_of(ap.parse_args(["--conf", "y"]), conf) == 0.0
    assert main.dist_weight_of(ap.parse_args(["--conf", "x", "--dist-weight", "0.5"]), conf) == 0.5
    for name in ("lego", "lego_4096", "fern"):  # the shipped configurations do not set it
        assert "DIST_WEIGHT" not in open(os.path.join(ROOT, "nerf-tiny_amd", "conf", name + ".ini")).read()
