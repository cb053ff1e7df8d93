"""No GPU: the restatements of rules VCG, VCU and VCT (tests/volume_compact_train_reference.py) against the dense restatements of VG, VU
and VT gathered at the rows, bit for bit, on volumes that carry garbage at their inactive points -- the premise of the device tests --,
and what the C entries and the package refuse without a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_compact_train_reference as T
import volume_grad_reference as V
import volume_reference as R
import volume_refine_reference as RF

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))
NRAYS = 120
DT = F(0.04)
BG = (0.25, 0.5, 1.0)
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def scene(shape):
    """make_volume with garbage sigma at its inactive points (the coefficients are random everywhere), rays, upstream values, and the
    dense restatement of VG on the garbage volume (computed once, never changed)"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        garbage, inactive = X.with_garbage(sigma, coef)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        G = V.geometry(garbage, coef, lo, step, o, d, tmin, tmax, DT)
        rng = np.random.default_rng(7)
        g_rgb, g_maps = rng.normal(0.0, 1.0, (NRAYS, 3)).astype(F), rng.normal(0.0, 1.0, (NRAYS, 2)).astype(F)
        _cache[shape] = dict(sigma=sigma, garbage=garbage, inactive=inactive, coef=coef, G=G, g_rgb=g_rgb, g_maps=g_maps,
                             index=R.active(garbage))
    return _cache[shape]


@pytest.mark.parametrize("t_stop", (0.0, 0.3))
@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_vcg_is_vg_gathered_at_the_rows(shape, degree, t_stop):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    index = s["index"]
    assert np.isnan(s["garbage"]).any() and (s["garbage"] < 0).any() and (coef[s["inactive"]] != 0).any()
    c = X.pack(s["garbage"], coef, False)
    assert np.array_equal(T.row_points(c), index)
    for g_maps in (None, s["g_maps"]):
        with np.errstate(all="ignore"):
            dense = V.reference(s["garbage"], coef, s["G"], s["g_rgb"], g_maps, BG, t_stop)
        got = T.reference(c, s["G"], s["g_rgb"], g_maps, BG, t_stop)
        want_S, want_C = T.gather(dense["dS"], dense["dC"].reshape(shape + (nc, 3)), index)
        assert np.array_equal(bits(got["dS"]), bits(want_S)) and np.array_equal(bits(got["dC"].reshape(len(index), -1)), bits(want_C))
        # the dense restatement on the garbage volume adds exactly 0 outside the list
        outside = np.ones(dense["dS"].size, bool)
        outside[index] = False
        assert not dense["dS"][outside].any() and not dense["dC"][outside].any()
        assert np.array_equal(got["valid"], dense["valid"]) and int(got["valid"].sum()) > 500 and np.count_nonzero(got["dC"]) > 50
    # a corner without a row receives nothing; the other rows keep what the dense restatement gives them
    hit = np.flatnonzero(got["dS"] != 0)
    r = int(hit[len(hit) // 2])
    slot = c.slot.copy()
    slot.reshape(-1)[index[r]] = -1 if degree else len(index)
    cb = c._replace(slot=slot)
    # (the dropped point keeps its values for the lookup: only the scatter is under test, so the samples are the whole volume's)
    sig, raw = T.lookup32(c, s["G"])
    col, mask = V.clamp_mask(raw)
    idx = V.pad(s["G"], sig)
    _, w, Tn, valid = V.forward(s["G"], sig, idx, np.float64, t_stop)
    dS, dC = T.vcg(cb, s["G"], idx, valid, w, Tn, col, mask, s["g_rgb"], s["g_maps"], BG)
    keep = np.arange(len(index)) != r
    assert dS[r] == 0 and not dC[r].any()
    assert np.array_equal(bits(dS[keep]), bits(got["dS"][keep])) and np.array_equal(bits(dC[keep]), bits(got["dC"][keep]))


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_vcu_is_vu_at_the_rows(shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    index = s["index"]
    n = len(index)
    c = X.pack(s["garbage"], coef, False)
    u_sigma, u_coef = X.unpack(c)
    rng = np.random.default_rng(3)
    sr, cr = rng.uniform(0.2, 3.0, n).astype(F), c.coef.copy()                 # every row alive (the smallest lattice has one positive point)
    sr[::7] = 0                                                                # but the dead rows
    u_sigma.reshape(-1)[index] = sr
    m_d, v_d = np.zeros((n, 1 + 3 * nc), F), np.zeros((n, 1 + 3 * nc), F)
    m_c, v_c = m_d.copy(), v_d.copy()
    for step in (1, 2, 3):
        aS_r = rng.integers(-2 ** 44, 2 ** 44, n)
        aC_r = rng.integers(-2 ** 44, 2 ** 44, (n, 3 * nc))
        aS_d, aC_d = np.zeros(shape, np.int64), np.zeros(shape + (nc, 3), np.int64)
        aS_d.reshape(-1)[index], aC_d.reshape(-1, 3 * nc)[index] = aS_r, aC_r
        V.vu_step(u_sigma, u_coef, index, aS_d, aC_d, m_d, v_d, 1.0 / 360, step, 2.0, 0.05)
        T.vcu_step(sr, cr, aS_r, aC_r, m_c, v_c, 1.0 / 360, step, 2.0, 0.05)
        gs, gc = T.gather(u_sigma, u_coef, index)
        assert np.array_equal(bits(sr), bits(gs)) and np.array_equal(bits(cr), bits(gc))
        assert np.array_equal(bits(m_c), bits(m_d)) and np.array_equal(bits(v_c), bits(v_d))
        assert not aS_r.any() and not aC_r.any()
    assert not sr[::7].any() and not m_c[::7, 0].any() and m_c[::7, 1:].any() and (sr > 0).any()
    assert (sr[1::7] == 0).any()                                               # the rate is large: a live sigma reached 0


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_vct_is_vt_gathered_at_the_rows(shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    index = s["index"]
    n = len(index)
    c = X.pack(s["garbage"], coef, False)
    u_sigma, u_coef = X.unpack(c)
    member = RF.member_mask(index, shape)
    for w_sigma, w_coef in ((0.7, 0.3), (0.0, 2.0), (3.0, 0.0), (0.0, 0.0)):
        aS_d, aC_d = np.zeros(shape, np.int64), np.zeros(shape + (nc, 3), np.int64)
        RF.vt(u_sigma, u_coef, index, member, w_sigma, w_coef, 1e-9, aS_d, aC_d)
        aS_r, aC_r = np.zeros(n, np.int64), np.zeros((n, 3 * nc), np.int64)
        T.vct(c, T.row_points(c), w_sigma, w_coef, 1e-9, aS_r, aC_r)
        want_S, want_C = T.gather(aS_d, aC_d, index)
        assert np.array_equal(aS_r, want_S) and np.array_equal(aC_r, want_C)
        assert aS_r.sum() == 0 and not aC_r.sum(0).any()                       # each word type's integers sum to exactly 0
        assert bool(aS_r.any()) == (w_sigma > 0) and bool(aC_r.any()) == (w_coef > 0)
    # a point list that disagrees with the slots: the rows whose point names another row receive nothing, the others what they did
    whole_S, whole_C = np.zeros(n, np.int64), np.zeros((n, 3 * nc), np.int64)
    T.vct(c, T.row_points(c), 0.7, 0.3, 1e-9, whole_S, whole_C)
    swapped = T.row_points(c)
    swapped[[1, n - 2]] = swapped[[n - 2, 1]]
    aS_r, aC_r = np.zeros(n, np.int64), np.zeros((n, 3 * nc), np.int64)
    T.vct(c, swapped, 0.7, 0.3, 1e-9, aS_r, aC_r)
    keep = np.ones(n, bool)
    keep[[1, n - 2]] = False
    assert not aS_r[~keep].any() and not aC_r[~keep].any() and whole_C[~keep].any()
    assert np.array_equal(aS_r[keep], whole_S[keep]) and np.array_equal(aC_r[keep], whole_C[keep])
    # a slot outside [0, n) is not a member: its row receives nothing and its neighbours' differences to it are 0
    slot = c.slot.copy()
    pts = index[[n // 3, 2 * n // 3]]
    slot.reshape(-1)[pts] = (n, -2)
    cb = c._replace(slot=slot)
    aS_r, aC_r = np.zeros(n, np.int64), np.zeros((n, 3 * nc), np.int64)
    T.vct(cb, T.row_points(c), 0.7, 0.3, 1e-9, aS_r, aC_r)
    ub_sigma, ub_coef = X.unpack(cb)
    aS_d, aC_d = np.zeros(shape, np.int64), np.zeros(shape + (nc, 3), np.int64)
    RF.vt(ub_sigma, ub_coef, index, RF.member_mask(np.setdiff1d(index, pts), shape), 0.7, 0.3, 1e-9, aS_d, aC_d)
    want_S, want_C = T.gather(aS_d, aC_d, index)
    assert np.array_equal(aS_r, want_S) and np.array_equal(aC_r, want_C) and not aS_r[[n // 3, 2 * n // 3]].any()


def test_c_entries_refuse_bad_arguments_without_a_device(pkg):
    """everything here is refused on the host before any device call; the pointers are never read"""
    L, f3 = pkg._abi.lib(), pkg._abi.f32_array
    p = 1 << 20                     # a non-null, 8-byte aligned stand-in
    lo, step, bg = f3([0.0] * 3), f3([1.0] * 3), f3([0.0] * 3)
    ERR = -1

    def backward(slot=p, srows=p, crows=p, n=5, occ=p, nx=5, degree=2, block=2, N=4, dt=0.1, t_stop=0.0, g_rgb=p, g_maps=None, acc_s=p, acc_c=p):
        return L.nerf_hip_volume_compact_render_backward(slot, srows, crows, n, occ, nx, 4, 3, degree, block, lo, step, p, p, p, p, N, dt, t_stop, bg,
                                                         g_rgb, g_maps, acc_s, acc_c, None)

    for kw in (dict(slot=None), dict(srows=None), dict(crows=None), dict(occ=None), dict(g_rgb=None), dict(acc_s=None), dict(acc_c=None),
               dict(acc_s=p + 4), dict(acc_c=p + 4), dict(crows=p + 2), dict(slot=p + 2), dict(g_maps=p + 2), dict(n=61), dict(n=-1), dict(nx=1),
               dict(degree=3), dict(degree=-1), dict(block=0), dict(N=-1), dict(dt=0.0), dict(dt=float("nan")), dict(t_stop=1.0),
               dict(n=0, acc_s=p + 4)):
        assert backward(**kw) == ERR and L.nerf_hip_last_error(), kw

    def adam(srows=p, crows=p, n=5, degree=2, acc_s=p, acc_c=p, m=p, v=p, grad_scale=1.0, step=1, lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8):
        return L.nerf_hip_volume_compact_adam_step(srows, crows, n, degree, acc_s, acc_c, m, v, grad_scale, step, lr, lr, beta1, beta2, eps, None)

    for kw in (dict(srows=None), dict(crows=None), dict(acc_s=None), dict(acc_c=None), dict(m=None), dict(v=None), dict(acc_s=p + 4),
               dict(acc_c=p + 4), dict(m=p + 2), dict(n=-1), dict(n=2 ** 31), dict(degree=3), dict(step=0), dict(grad_scale=float("inf")),
               dict(lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(eps=float("inf"))):
        assert adam(**kw) == ERR and L.nerf_hip_last_error(), kw
    assert adam(n=0, srows=None, crows=None, acc_s=None, acc_c=None, m=None, v=None) == 0      # no rows: nothing is launched

    def tv(slot=p, srows=p, crows=p, point=p, n=5, nx=5, degree=2, w_sigma=1.0, w_coef=1.0, eps=1e-9, acc_s=p, acc_c=p):
        return L.nerf_hip_volume_compact_tv_backward(slot, srows, crows, point, n, nx, 4, 3, degree, w_sigma, w_coef, eps, acc_s, acc_c, None)

    for kw in (dict(slot=None), dict(srows=None), dict(crows=None), dict(point=None), dict(acc_s=None), dict(acc_c=None), dict(acc_s=p + 4),
               dict(acc_c=p + 4), dict(point=p + 2), dict(n=61), dict(n=-1), dict(nx=1), dict(degree=3), dict(w_sigma=-1.0),
               dict(w_coef=65537.0), dict(w_sigma=float("nan")), dict(eps=0.0), dict(eps=float("inf"))):
        assert tv(**kw) == ERR and L.nerf_hip_last_error(), kw
    assert tv(w_sigma=0.0, w_coef=0.0) == 0 and tv(n=0, srows=None, crows=None, point=None, acc_s=None, acc_c=None) == 0
    assert backward(n=0, srows=None, crows=None, acc_s=None, acc_c=None) == 0 and backward(N=0) == 0


def compact_on_cpu(pkg, degree=2, half=False):
    n = 5
    return pkg.volume.CompactVolume(torch.full((5, 4, 3), -1, dtype=torch.int32), torch.zeros(n), torch.zeros(n, X.row_width(degree, half),
                                    dtype=torch.float16 if half else torch.float32), torch.zeros(2, 2, 1, dtype=torch.uint8),
                                    np.zeros(3, F), np.ones(3, F), 2, degree, (5, 4, 3))


def test_python_calls_refuse_cpu_tensors_and_dense_volumes(pkg):
    V_ = pkg.volume
    c = compact_on_cpu(pkg)
    dense = V_.Volume(torch.zeros(5, 4, 3), torch.zeros(5, 4, 3, 9, 3), torch.zeros(2, 2, 1, dtype=torch.uint8), np.zeros(3, F), np.ones(3, F), 2, 2)
    z = torch.zeros(4, 3)
    grad = V_.CompactGrad(torch.zeros(5, dtype=torch.int64), torch.zeros(5, 27, dtype=torch.int64))
    calls = lambda v: [lambda: V_.compact_grad_buffers(v), lambda: V_.compact_render_backward(v, grad, z, z, 0.0, 1.0, z),
                       lambda: V_.compact_tv_backward(v, grad, 1.0, 1.0), lambda: V_.row_points(v), lambda: V_.CompactFinetuner(v),
                       lambda: V_.finetune_compact(v, None, None, 1)]
    for call in calls(c):
        with pytest.raises(RuntimeError, match="runs only on a ROCm device"):
            call()
    for call in calls(dense):
        with pytest.raises(TypeError, match="CompactVolume"):
            call()
    # the dense calls still refuse the compact form
    with pytest.raises(TypeError, match="unpack"):
        V_.Finetuner(c)


def test_runner_and_driver_options(pkg):
    import importlib

    bake = pkg.NeRFRunner.bake_volume
    for kw in (dict(finetune=2), dict(compact="fp16"), dict(compact="fp16", finetune=0), dict()):
        with pytest.raises(ValueError, match="finetune_compact"):
            bake(types.SimpleNamespace(), 8, finetune_compact=True, **kw)          # refused before the runner is looked at
    ap = importlib.import_module("nerf_tiny_amd.main").build_parser()
    a = ap.parse_args(["--volume", "24", "--volume-compact", "fp16", "--volume-finetune", "3", "--volume-finetune-compact"])
    assert a.volume_finetune_compact is True and ap.parse_args(["--volume", "24"]).volume_finetune_compact is False


def test_header_and_abi(pkg):
    hdr = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define NERF_HIP_ABI_VERSION 7\b", hdr)
    for text in ("VCG. THE GRADIENT OF THE COMPACT MARCH", "VCU. THE UPDATE OVER ROWS", "VCT. TOTAL VARIATION OVER ROWS"):
        assert text in hdr, text
    lib = pkg._abi.lib()
    for name in ("render_backward", "adam_step", "tv_backward"):
        full = "nerf_hip_volume_compact_" + name
        assert re.search(r"\b" + full + r"\(", hdr) and full in pkg._abi.EXPORTS and hasattr(lib, full), name
    for name in ("CompactGrad", "compact_grad_buffers", "compact_render_backward", "compact_tv_backward", "row_points", "CompactFinetuner",
                 "finetune_compact"):
        assert hasattr(pkg.volume, name), name
