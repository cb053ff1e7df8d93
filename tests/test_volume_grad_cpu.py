"""No GPU: the restatements of rules VG and VU (tests/volume_grad_reference.py) against torch.autograd and torch.optim.Adam in fp64, the
error budget's teeth, and the learning case the GPU test repeats through volume.Finetuner."""
import os
import re

import numpy as np
import pytest
import torch

import volume_grad_reference as V
import volume_reference as R

F = np.float32
BG = (0.25, 0.5, 1.0)
DT = F(0.04)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def scene(shape, degree=2, nrays=300):
    key = (shape, degree, nrays)
    if key not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        coef = np.ascontiguousarray(coef[..., :(degree + 1) ** 2, :])
        o, d, tmin, tmax = R.make_rays(nrays, 5, lo, step, shape)
        G = V.geometry(sigma, coef, lo, step, o, d, tmin, tmax, DT)
        rng = np.random.default_rng(7)
        g_rgb = rng.normal(0.0, 1.0, (nrays, 3)).astype(F)
        g_maps = rng.normal(0.0, 1.0, (nrays, 2)).astype(F)
        _cache[key] = dict(sigma=sigma, coef=coef, G=G, g_rgb=g_rgb, g_maps=g_maps)
    return _cache[key]


# ---- VG against autograd ----

def _lerp(a, b, f):
    return a + f * (b - a)


def _tri(v, f):
    """v [M, 2, 2, 2, ...], f [M, 3]: z first, then y, then x"""
    ex = (slice(None),) + (None,) * (v.dim() - 4)
    c = _lerp(v[:, :, :, 0], v[:, :, :, 1], f[:, 2][ex][:, None, None])
    c = _lerp(c[:, :, 0], c[:, :, 1], f[:, 1][ex][:, None])
    return _lerp(c[:, 0], c[:, 1], f[:, 0][ex])


def _corners(a, ci):
    i, j, k = ci[:, 0], ci[:, 1], ci[:, 2]
    return torch.stack([torch.stack([torch.stack([a[i + di, j + dj, k + dk] for dk in (0, 1)], 1) for dj in (0, 1)], 1) for di in (0, 1)], 1)


def torch_march(sigma, coef, G, bg, t_stop):
    """A differentiable fp64 restatement of VL + VR at G's samples -> (rgb [N, 3], maps [N, 2]) and, detached, what VG's closed form
    takes: idx, valid, w, Tn, c, mask."""
    nc = coef.shape[3]
    ci = torch.from_numpy(G.ci)
    f = torch.from_numpy(G.f.astype(np.float64))
    inside = torch.from_numpy(G.inside)
    sig = torch.where(inside, _tri(_corners(sigma, ci), f), torch.zeros((), dtype=torch.float64))
    Y = torch.from_numpy(G.Y.astype(np.float64))[torch.from_numpy(G.rid)][:, :nc]
    raw = _tri((Y[:, None, None, None, :, None] * _corners(coef, ci)).sum(-2), f)
    c = raw.clamp(0.0, 1.0)
    idx = V.pad(G, sig.detach().numpy())
    N, Mx = idx.shape
    tk = torch.from_numpy(G.tk.astype(np.float64))
    T = torch.ones(N, dtype=torch.float64)
    alive = torch.ones(N, dtype=torch.bool)
    C, D, A = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    ws, Ts, vs = [], [], []
    for i in range(Mx):
        col = torch.from_numpy(idx[:, i])
        on = alive & (col >= 0)
        j = col.clamp(min=0)
        alpha = -torch.expm1(-(sig[j] * float(G.dt)))
        w = torch.where(on, T * alpha, torch.zeros((), dtype=torch.float64))
        C = C + w[:, None] * c[j]
        D = D + w * tk[j]
        A = A + w
        T = T - w
        ws.append(w.detach()), Ts.append(T.detach().clone()), vs.append(on.clone())
        alive = on & ~(T.detach() < t_stop)
    rgb = C + (1.0 - A)[:, None] * torch.tensor(bg, dtype=torch.float64)
    st = lambda a: torch.stack(a, 1).numpy()
    raw_np = raw.detach().numpy()
    mask = (raw_np >= 0) & (raw_np <= 1)
    return rgb, torch.stack([D, A], 1), dict(idx=idx, valid=st(vs), w=st(ws), Tn=st(Ts), c=c.detach().numpy(), mask=mask)


@pytest.mark.parametrize("t_stop", (0.0, 0.3))
@pytest.mark.parametrize("with_maps", (False, True))
@pytest.mark.parametrize("degree", (0, 1, 2))
def test_closed_form_is_autograd(degree, with_maps, t_stop):
    s = scene((9, 8, 7), degree, 120)
    G = s["G"]
    sigma = torch.from_numpy(s["sigma"].astype(np.float64)).requires_grad_(True)
    coef = torch.from_numpy(s["coef"].astype(np.float64)).requires_grad_(True)
    rgb, maps, fw = torch_march(sigma, coef, G, BG, t_stop)
    g_rgb, g_maps = s["g_rgb"][:120], (s["g_maps"][:120] if with_maps else None)
    L = (rgb * torch.from_numpy(g_rgb.astype(np.float64))).sum()
    if with_maps:
        L = L + (maps * torch.from_numpy(g_maps.astype(np.float64))).sum()
    a_sigma, a_coef = torch.autograd.grad(L, (sigma, coef))
    dS, dC = V.vg(G, fw["idx"], fw["valid"], fw["w"], fw["Tn"], fw["c"], fw["mask"], g_rgb, g_maps, BG, coef.shape[3])
    es = np.abs(dS - a_sigma.numpy().reshape(-1)).max()
    ec = np.abs(dC - a_coef.numpy().reshape(dC.shape)).max()
    scale = max(np.abs(dS).max(), np.abs(dC).max())
    print(f"degree {degree} maps {with_maps} t_stop {t_stop}: closed form vs autograd {es:.2e} / {ec:.2e} at scale {scale:.2e}")
    assert scale > 1e-2 and es <= 1e-12 * scale and ec <= 1e-12 * scale
    if t_stop:
        full = V.pad(G, V.lookup32(s["sigma"], s["coef"], G)[0])
        assert fw["valid"].sum() < (full >= 0).sum()                    # some rays are truncated
    assert (~fw["mask"][fw["idx"][fw["valid"]]]).any() and fw["mask"][fw["idx"][fw["valid"]]].any()


# ---- VU against torch.optim.Adam ----

def test_update_is_adam():
    shape, degree = (5, 4, 3), 1
    sigma, coef, _, _ = R.make_volume(shape, seed=11, degree=degree)
    index = R.active(sigma)
    nc = coef.shape[3]
    words = 1 + 3 * nc
    rng = np.random.default_rng(3)
    m, v = np.zeros((index.size, words), F), np.zeros((index.size, words), F)
    x0 = np.concatenate([sigma.reshape(-1)[index][:, None], coef.reshape(-1, 3 * nc)[index]], 1)
    live = np.ones(x0.shape, bool)
    live[:, 0] = x0[:, 0] > 0
    assert live[:, 0].any() and (~live[:, 0]).any()
    lr_s, lr_c, scale = 1e-3, 1e-2, 1.0 / 192
    p = torch.tensor(x0.astype(np.float64), requires_grad=True)
    lrs = torch.tensor([lr_s] + [lr_c] * (3 * nc), dtype=torch.float64)
    # one Adam per rate: torch's update is elementwise, so two optimisers over two leaves restate the two rates
    ps = p.detach()[:, :1].clone().requires_grad_(True)
    pc = p.detach()[:, 1:].clone().requires_grad_(True)
    opt = [torch.optim.Adam([ps], lr=lr_s, betas=(0.9, 0.999), eps=1e-8), torch.optim.Adam([pc], lr=lr_c, betas=(0.9, 0.999), eps=1e-8)]
    del p, lrs
    sg, cf = sigma.copy(), coef.copy()
    for step in (1, 2, 3):
        aS = np.zeros(sigma.size, np.int64)
        aC = np.zeros((sigma.size, 3 * nc), np.int64)
        aS[index] = rng.integers(-2 ** 44, 2 ** 44, index.size)
        aC[index] = rng.integers(-2 ** 44, 2 ** 44, (index.size, 3 * nc))
        g = np.concatenate([aS[index][:, None], aC[index]], 1).astype(np.float64) * 2.0 ** -40 * scale
        ps.grad, pc.grad = torch.from_numpy(g[:, :1].copy()), torch.from_numpy(g[:, 1:].copy())
        for o in opt:
            o.step()
        V.vu_step(sg, cf, index, aS, aC, m, v, scale, step, lr_s, lr_c)
        assert not aS.any() and not aC.any()
    x = np.concatenate([sg.reshape(-1)[index][:, None], cf.reshape(-1, 3 * nc)[index]], 1)
    want = np.concatenate([ps.detach().numpy(), pc.detach().numpy()], 1)
    # fp32 rounding: x once per step (2^-24 |x|), m' and v' once per step (each moves the update by a few 2^-24 of itself, |update| < 4 lr)
    tol = 3 * (2.0 ** -24 * np.abs(x0).max() + 32 * 2.0 ** -24 * lr_c)
    assert np.abs(x - want)[live].max() <= tol and np.abs(x - x0)[live].min() > 0
    # dead points keep x, m and v (their coefficient words are updated like any other)
    dead = ~live[:, 0]
    assert np.array_equal(x[dead, 0], x0[dead, 0]) and not m[dead, 0].any() and not v[dead, 0].any() and m[dead, 1:].all()
    # outside the list nothing moves
    out = np.ones(sigma.size, bool)
    out[index] = False
    assert np.array_equal(cf.reshape(-1, 3 * nc)[out], coef.reshape(-1, 3 * nc)[out])


# ---- the budget has teeth ----

def test_inputs_are_what_the_gpu_test_states():
    s = scene((9, 8, 7))
    ref = V.reference(s["sigma"], s["coef"], s["G"], s["g_rgb"], s["g_maps"], BG)
    assert R.active(s["sigma"]).size == 130 and s["sigma"].size == 504 and int((s["sigma"] > 0).sum()) == 24
    clamped = ~ref["mask"][ref["idx"][ref["valid"]]]
    assert abs(clamped.mean() - 0.043) < 0.0005, clamped.mean()


@pytest.mark.parametrize("t_stop", (0.0, 0.3))
def test_budget_with_teeth(t_stop):
    s = scene((9, 8, 7))
    G, nc = s["G"], 9
    sig, raw = V.lookup32(s["sigma"], s["coef"], G)
    c, mask = V.clamp_mask(raw)
    idx = V.pad(G, sig)
    _, w32, T32, valid32 = V.forward(G, sig, idx, np.float32, t_stop)
    limit = valid32.sum(1)                                                 # the fp32 forward's own contributing counts
    ref = V.reference(s["sigma"], s["coef"], G, s["g_rgb"], s["g_maps"], BG, t_stop=0.0, limit=limit)
    assert np.array_equal(ref["valid"], valid32[:, :ref["valid"].shape[1]])
    args = (s["g_rgb"], s["g_maps"], BG, nc)
    honest = V.worst_ratio(*V.vg(G, idx, valid32, w32, T32, c, mask, *args), ref)
    print(f"t_stop {t_stop}: fp32 forward vs fp64 restatement, worst error / budget = {honest:.3f}")
    assert honest <= 1.0
    if t_stop:
        assert limit.sum() < (idx >= 0).sum()
    # one contributing sample dropped from one ray
    r = int(np.flatnonzero(limit >= 3)[0])
    idx_d = V.pad(G, sig, drop=(r, 1))
    _, wd, Td, vd = V.forward(G, sig, idx_d, np.float32, t_stop)
    wrong = {"drop": V.worst_ratio(*V.vg(G, idx_d, vd, wd, Td, c, mask, *args), ref)}
    # dt scaled by 1 + 2^-10
    dt2 = F(np.float64(G.dt) * (1 + 2.0 ** -10))
    _, w2, T2, v2 = V.forward(G, sig, idx, np.float32, t_stop, dt=dt2)
    wrong["dt"] = V.worst_ratio(*V.vg(G, idx, v2 & valid32, w2, T2, c, mask, *args, dt=dt2), ref)
    for mut in ("P_exclusive", "no_mask", "no_bg"):
        wrong[mut] = V.worst_ratio(*V.vg(G, idx, valid32, w32, T32, c, mask, *args, mutate=mut), ref)
    print({k: f"{x:.3g}" for k, x in wrong.items()})
    assert all(x > 1.0 for x in wrong.values()), wrong


# ---- the learning case ----

def test_learning_in_the_restatement():
    case = V.learning_case()
    losses, sigma, coef = V.learn(case)
    print(f"restatement: loss {losses[0]:.3e} -> {losses[-1]:.3e} ({losses[-1] / losses[0]:.4f})")
    assert losses[0] > 1e-4 and losses[-1] <= 0.25 * losses[0]
    # the frozen support: nothing outside the baked active list moved, no sigma went from 0 to positive
    out = np.ones(sigma.size, bool)
    out[case["index"]] = False
    assert np.array_equal(sigma.reshape(-1)[out], case["s2"].reshape(-1)[out]) and not (sigma[case["s2"] == 0] != 0).any()
    assert np.array_equal(coef.reshape(-1, 27)[out], case["c2"].reshape(-1, 27)[out])


# ---- the surface ----

def test_abi_declares_the_two_calls(pkg):
    hdr = open(os.path.join(ROOT, "include", "nerf_hip.h")).read()
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr) and pkg._abi.NERF_HIP_ABI_VERSION == 7
    assert re.search(r"#define\s+NERF_HIP_VOLUME_GRAD_SHIFT\s+40\b", hdr) and pkg._abi.VOLUME_GRAD_SHIFT == 40 == V.SHIFT
    lib = pkg._abi.lib()
    for name in ("nerf_hip_volume_render_backward", "nerf_hip_volume_adam_step"):
        assert re.search(r"\b" + name + r"\(", hdr) and name in pkg._abi.EXPORTS and hasattr(lib, name), name
    for name in ("grad_buffers", "render_backward", "gradients", "render_train", "Finetuner", "finetune", "VolumeGrad"):
        assert hasattr(pkg.volume, name), name


def test_cpu_tensors_are_refused(pkg):
    sigma, coef, lo, step = R.make_volume((5, 4, 3), seed=11)
    t = torch.from_numpy
    vol = pkg.volume.Volume(t(sigma), t(coef), torch.zeros(2, 2, 1, dtype=torch.uint8), lo, step, 2, 2)
    z = torch.zeros(4, 3)
    for call in (lambda: pkg.volume.grad_buffers(vol), lambda: pkg.volume.Finetuner(vol),
                 lambda: pkg.volume.render_train(vol, z, z, 0.0, 1.0),
                 lambda: pkg.volume.render_backward(vol, None, z, z, 0.0, 1.0, z)):
        with pytest.raises(RuntimeError):
            call()
