"""GPU: the backward pass of the SH volume march and the volume Adam step (csrc/volume_grad.hip; rules VG and VU) against the fp64
restatement and its derived word-by-word budget (tests/volume_grad_reference.py), bit for bit wherever the rule promises it, through
torch.autograd, volume.Finetuner and the runner; refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import volume_grad_reference as V
import volume_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))
BLOCKS = (1, 2, 4, 8, 1 << 30)                   # the last: one block
NRAYS = 300
DT = F(0.04)                                     # at most 71 samples a ray
BG = (0.25, 0.5, 1.0)
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view({4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def scene(shape):
    """the hand-made volume of a lattice, its rays, their geometry and the upstream values (computed once, never changed)"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        G = V.geometry(sigma, coef, lo, step, o, d, tmin, tmax, DT)
        rng = np.random.default_rng(7)
        g_rgb = rng.normal(0.0, 1.0, (NRAYS, 3)).astype(F)
        g_maps = rng.normal(0.0, 1.0, (NRAYS, 2)).astype(F)
        _cache[shape] = dict(sigma=sigma, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax, G=G, g_rgb=g_rgb, g_maps=g_maps)
    return _cache[shape]


def device_volume(pkg, dev, s, block, degree=2):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sigma = t(s["sigma"])
    nc = (degree + 1) ** 2
    return pkg.volume.Volume(sigma, t(s["coef"][..., :nc, :]), pkg.volume.blocks(sigma, block), s["lo"], s["step"],
                             min(block, pkg.volume.ONE_BLOCK), degree)


def rays_on(dev, s, sel=slice(None)):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    return t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"])


def backward(pkg, dev, s, vol, sel=slice(None), grad=None, t_stop=0.0, maps=True, g_rgb=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    grad = pkg.volume.grad_buffers(vol) if grad is None else grad
    return pkg.volume.render_backward(vol, grad, *rays_on(dev, s, sel), t(s["g_rgb"] if g_rgb is None else g_rgb),
                                      t(s["g_maps"]) if maps else None, dt=DT, t_stop=t_stop, background=BG)


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_accumulators_within_the_budget(pkg, dev, shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    vol = device_volume(pkg, dev, s, 2, degree)
    for t_stop in (0.0, 0.3):
        steps = pkg.volume.render(vol, *rays_on(dev, s), dt=DT, t_stop=t_stop, background=BG)[2].cpu().numpy()
        ref = V.reference(s["sigma"], coef, s["G"], s["g_rgb"], s["g_maps"], BG, limit=steps[:, 0])
        assert np.array_equal(ref["valid"].sum(1), steps[:, 0])               # the restatement sees the device's contributing samples
        if t_stop:
            full = V.pad(s["G"], ref["sig"])
            assert (steps[:, 0] < (full >= 0).sum(1)).any()                   # some rays are truncated
        grad = backward(pkg, dev, s, vol, t_stop=t_stop)
        got_S = grad.acc_sigma.cpu().numpy().astype(np.float64) * 2.0 ** -V.SHIFT
        got_C = grad.acc_coef.cpu().numpy().astype(np.float64) * 2.0 ** -V.SHIFT
        worst = V.worst_ratio(got_S, got_C, ref)
        print(f"{shape} degree {degree} t_stop {t_stop}: device accumulators vs fp64 restatement, worst error / budget = {worst:.4f}")
        assert worst <= 1.0
        assert np.abs(got_S).max() > 1e-2 and np.abs(got_C).max() > 1e-2
        # gradients(): the same words read as fp32
        d_sigma, d_coef = pkg.volume.gradients(grad, scale=0.5)
        assert np.array_equal(bits(d_sigma), bits((got_S * 0.5).astype(F).reshape(shape)))
        assert np.array_equal(bits(d_coef), bits((got_C * 0.5).astype(F).reshape(shape + (nc, 3))))
        if shape == (9, 8, 7) and degree == 2 and not t_stop:
            # what the inputs hold, so that a clamp bug cannot hide
            assert R.active(s["sigma"]).size == 130 and s["sigma"].size == 504 and int((s["sigma"] > 0).sum()) == 24
            clamped = ~ref["mask"][ref["idx"][ref["valid"]]]
            assert abs(clamped.mean() - 0.043) < 0.0005
        # exact zero outside the active list
        out = np.ones(s["sigma"].size, bool)
        out[R.active(s["sigma"])] = False
        assert not got_S.reshape(-1)[out].any() and not got_C.reshape(-1, 3 * nc)[out].any()


@pytest.mark.parametrize("shape", LATTICES)
def test_bit_for_bit(pkg, dev, shape):
    s = scene(shape)
    vol = device_volume(pkg, dev, s, 2)
    base = backward(pkg, dev, s, vol, t_stop=0.3)
    same = lambda g: np.array_equal(bits(g.acc_sigma), bits(base.acc_sigma)) and np.array_equal(bits(g.acc_coef), bits(base.acc_coef))
    assert base.acc_sigma.any() and base.acc_coef.any()
    assert same(backward(pkg, dev, s, vol, t_stop=0.3))                                      # the same call twice
    perm = np.random.default_rng(1).permutation(NRAYS)
    assert same(backward(pkg, dev, s, vol, sel=perm, t_stop=0.3))                            # the rays permuted
    two = backward(pkg, dev, s, vol, sel=slice(0, 130), t_stop=0.3)
    assert not same(two)
    assert same(backward(pkg, dev, s, vol, sel=slice(130, NRAYS), grad=two, t_stop=0.3))     # two accumulating calls
    for B in BLOCKS:
        assert same(backward(pkg, dev, s, device_volume(pkg, dev, s, B), t_stop=0.3)), B     # every block edge


def test_zeros(pkg, dev):
    s = scene((9, 8, 7))
    vol = device_volume(pkg, dev, s, 2)
    none = lambda g: not g.acc_sigma.any() and not g.acc_coef.any()
    assert none(backward(pkg, dev, s, vol, sel=slice(0, 0)))                                 # 0 rays
    hits = np.zeros(NRAYS, bool)
    hits[np.unique(s["G"].rid)] = True
    miss = np.flatnonzero(~hits)
    assert miss.size >= NRAYS // 10 and 0 in miss                                            # the NaN origin among them
    assert none(backward(pkg, dev, s, vol, sel=miss))
    # a NaN (or inf) upstream value silences its ray, and only its ray
    ref = V.reference(s["sigma"], s["coef"], s["G"], s["g_rgb"], s["g_maps"], BG)
    r = int(np.flatnonzero(ref["valid"].sum(1) >= 3)[0])
    for bad, ch in ((np.nan, 1), (np.inf, 2)):
        g = s["g_rgb"].copy()
        g[r, ch] = bad
        assert none(backward(pkg, dev, s, vol, sel=slice(r, r + 1), g_rgb=g))
        rest = np.delete(np.arange(NRAYS), r)
        a, b = backward(pkg, dev, s, vol, g_rgb=g), backward(pkg, dev, s, vol, sel=rest)
        assert np.array_equal(bits(a.acc_sigma), bits(b.acc_sigma)) and np.array_equal(bits(a.acc_coef), bits(b.acc_coef)) and not none(a)
    gm = {**s, "g_maps": s["g_maps"].copy()}
    gm["g_maps"][r, 0] = np.nan
    assert none(backward(pkg, dev, gm, vol, sel=slice(r, r + 1))) and not none(backward(pkg, dev, s, vol, sel=slice(r, r + 1)))


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_update_is_the_restatement(pkg, dev, degree):
    shape = (9, 8, 7)
    s = scene(shape)
    nc = (degree + 1) ** 2
    vol = device_volume(pkg, dev, s, 2, degree)
    sigma, coef = s["sigma"].copy(), np.ascontiguousarray(s["coef"][..., :nc, :]).copy()
    index = R.active(sigma)
    d_index = pkg.volume.active(vol.sigma)
    assert np.array_equal(d_index.cpu().numpy(), index)
    words = 1 + 3 * nc
    m, v = np.zeros((index.size, words), F), np.zeros((index.size, words), F)
    d_sigma, d_coef = vol.sigma.clone(), vol.coef.clone()
    d_m, d_v = torch.zeros(index.size, words, device=dev), torch.zeros(index.size, words, device=dev)
    rng = np.random.default_rng(9)
    for step in (1, 2, 3):
        aS = np.zeros(sigma.size, np.int64)
        aC = np.zeros((sigma.size, 3 * nc), np.int64)
        aS[index] = rng.integers(-2 ** 46, 2 ** 46, index.size)                # with a rate of 3 some sigmas reach 0
        aC[index] = rng.integers(-2 ** 42, 2 ** 42, (index.size, 3 * nc))
        aC[index[::5], 0] = 0                                                  # words that receive nothing
        d_aS, d_aC = torch.from_numpy(aS.reshape(shape)).to(dev), torch.from_numpy(aC.reshape(shape + (nc, 3))).to(dev)
        pkg.ops.volume_adam_step(d_sigma, d_coef, d_index, d_aS, d_aC, d_m, d_v, 1.0 / 192, step, 3.0, 0.01)
        V.vu_step(sigma, coef, index, aS, aC, m, v, 1.0 / 192, step, 3.0, 0.01)
        assert not d_aS.any() and not d_aC.any()
        for got, want in ((d_sigma, sigma), (d_coef, coef), (d_m, m), (d_v, v)):
            assert np.array_equal(bits(got), bits(want)), step
    dead = s["sigma"].reshape(-1)[index] == 0
    assert dead.any() and not m[dead, 0].any() and m[~dead, 0].all()
    assert ((sigma == 0) & (s["sigma"] > 0)).any()                             # a point died on the way, and stayed dead
    assert np.array_equal(bits(vol.sigma), bits(s["sigma"]))                   # the input was not touched


def test_autograd(pkg, dev):
    s = scene((9, 8, 7))
    vol = device_volume(pkg, dev, s, 2)
    rays = rays_on(dev, s)
    g_rgb, g_maps = torch.from_numpy(s["g_rgb"]).to(dev), torch.from_numpy(s["g_maps"]).to(dev)
    plain = pkg.volume.render(vol, *rays, dt=DT, t_stop=1e-3, background=BG)
    tv = vol._replace(sigma=vol.sigma.clone().requires_grad_(True), coef=vol.coef.clone().requires_grad_(True))
    rgb, maps, steps = pkg.volume.render_train(tv, *rays, dt=DT, t_stop=1e-3, background=BG)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((rgb, maps, steps), plain))
    assert rgb.requires_grad and maps.requires_grad and not steps.requires_grad
    gs, gc = torch.autograd.grad((rgb * g_rgb).sum() + (maps * g_maps).sum(), (tv.sigma, tv.coef))
    grad = pkg.volume.render_backward(vol, pkg.volume.grad_buffers(vol), *rays, g_rgb, g_maps, dt=DT, t_stop=1e-3, background=BG)
    ws, wc = pkg.volume.gradients(grad)
    assert np.array_equal(bits(gs), bits(ws)) and np.array_equal(bits(gc), bits(wc)) and gs.any() and gc.any()
    # rgb alone: the maps' upstream is absent
    rgb2 = pkg.volume.render_train(tv, *rays, dt=DT, t_stop=1e-3, background=BG)[0]
    gs2, gc2 = torch.autograd.grad((rgb2 * g_rgb).sum(), (tv.sigma, tv.coef))
    grad2 = pkg.volume.render_backward(vol, pkg.volume.grad_buffers(vol), *rays, g_rgb, None, dt=DT, t_stop=1e-3, background=BG)
    ws2, wc2 = pkg.volume.gradients(grad2)
    assert np.array_equal(bits(gs2), bits(ws2)) and np.array_equal(bits(gc2), bits(wc2)) and not np.array_equal(bits(gs2), bits(gs))


def test_learning(pkg, dev):
    """volume_grad_reference.learning_case through Finetuner: 25 full-batch steps at the default rates.
    The factor 2 against the restatement's own final loss is there because the two trajectories are not comparable bit by bit (fp32
    against fp64 forward, quantised against unquantised sums); it is not a measured margin."""
    case = V.learning_case()
    want, _, _ = V.learn(case)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sigma = t(case["s2"])
    vol = pkg.volume.Volume(sigma, t(case["c2"]), pkg.volume.blocks(sigma, 2), case["lo"], case["step"], 2, 2)
    keep = [vol.sigma.clone(), vol.coef.clone()]
    tuner = pkg.volume.Finetuner(vol)
    rays = (t(case["o"]), t(case["d"]), t(case["tmin"]), t(case["tmax"]))
    target = t(case["target"])
    losses = [tuner.step(*rays, target, background=V.LEARN_BG, dt=V.LEARN_DT, t_stop=0.0) for _ in range(V.LEARN_STEPS)]
    assert all(l.is_cuda and l.dim() == 0 for l in losses) and tuner.steps == V.LEARN_STEPS
    out = tuner.volume()
    final = float(((pkg.volume.render(out, *rays, dt=V.LEARN_DT, t_stop=0.0, background=V.LEARN_BG)[0] - target) ** 2).mean())
    first = float(losses[0])
    print(f"Finetuner: loss {first:.3e} -> {final:.3e} ({final / first:.4f}); the restatement: {want[0]:.3e} -> {want[-1]:.3e}")
    assert abs(first - want[0]) <= 1e-3 * want[0]
    assert final <= 0.25 * first and final <= 2.0 * want[-1]
    assert np.array_equal(bits(vol.sigma), bits(keep[0])) and np.array_equal(bits(vol.coef), bits(keep[1]))
    assert np.array_equal(out.occ.cpu().numpy(), pkg.volume.blocks(out.sigma, out.block).cpu().numpy())
    assert np.array_equal(out.occ.cpu().numpy(), R.blocks(out.sigma.cpu().numpy(), 2)) and (out.block, out.degree) == (2, 2)
    # the frozen support
    outside = np.ones(case["s2"].size, bool)
    outside[case["index"]] = False
    assert np.array_equal(bits(out.sigma).reshape(-1)[outside], bits(vol.sigma).reshape(-1)[outside])
    assert not (out.sigma[vol.sigma == 0] != 0).any() and not tuner.grad.acc_sigma.any() and not tuner.grad.acc_coef.any()


def test_runner_finetunes_saves_and_reports(pkg, dev, tmp_path, capsys):
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    rs = str(tmp_path) + "/rs/"
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=20, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=20)
    run.trainer("train")
    capsys.readouterr()
    vol = run.bake_volume(24, degree=1, finetune=5, finetune_batch=128)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("[VOLUME]")]
    assert len(lines) == 2 and "finetune" in lines[1] and "5 steps" in lines[1] and "loss" in lines[1]
    plain = glob.glob(rs + "*_volume24.npz")
    tuned = glob.glob(rs + "*_volume24_ft5.npz")
    assert len(plain) == 1 and len(tuned) == 1 and os.path.basename(tuned[0]) == f"{run.start_time}_{run.last_iter}_volume24_ft5.npz"
    back, baked = pkg.volume.load(tuned[0], dev), pkg.volume.load(plain[0], dev)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(back[:3], vol[:3])) and back.degree == 1
    assert not np.array_equal(bits(back.coef), bits(baked.coef))
    ft = run.last_volume_finetune
    assert ft["iters"] == 5 and np.isfinite(ft["first_loss"]) and np.isfinite(ft["last_loss"])
    # with a preview: the scores against the split's own images before and after; without the arguments nothing new happens
    run.bake_volume(24, degree=1, finetune=2, finetune_batch=128, finetune_lr=(0.05, 0.005), preview="train", save=False)
    out = capsys.readouterr().out
    assert out.count("[VOLUME]") == 3 and "ground truth" in out and out.count("[PSNR]") == 2
    run.bake_volume(24, degree=1, save=False)
    assert capsys.readouterr().out.count("[VOLUME]") == 1 and len(glob.glob(rs + "*_ft*.npz")) == 1
    with pytest.raises(ValueError):
        run.bake_volume(24, finetune=-1)


def test_refusals(pkg, dev):
    L, abi = pkg._abi.lib(), pkg._abi
    s = scene((5, 4, 3))
    vol = device_volume(pkg, dev, s, 2)
    nx, ny, nz = 5, 4, 3
    f3 = abi.f32_array
    lo, step, bg = s["lo"].tolist(), s["step"].tolist(), [0.0, 0.0, 0.0]
    n = 4
    o, d = torch.zeros(n, 3, device=dev), torch.ones(n, 3, device=dev)
    t0, t1 = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    g, gm = torch.zeros(n, 3, device=dev), torch.zeros(n, 2, device=dev)
    grad = pkg.volume.grad_buffers(vol)
    index = pkg.volume.active(vol.sigma)
    na = int(index.shape[0])
    m, v = torch.zeros(na, 28, device=dev), torch.zeros(na, 28, device=dev)
    sg, cf = vol.sigma.clone(), vol.coef.clone()
    P = lambda t: t.data_ptr()

    def back(**kw):
        a = dict(sigma=P(vol.sigma), coef=P(vol.coef), occ=P(vol.occ), nx=nx, ny=ny, nz=nz, degree=2, block=2, lo=lo, step=step, o=P(o), d=P(d),
                 tmin=P(t0), tmax=P(t1), N=n, dt=0.1, t_stop=0.0, bg=bg, g=P(g), gm=P(gm), aS=P(grad.acc_sigma), aC=P(grad.acc_coef))
        a.update(kw)
        return L.nerf_hip_volume_render_backward(a["sigma"], a["coef"], a["occ"], a["nx"], a["ny"], a["nz"], a["degree"], a["block"], f3(a["lo"]),
                                                 f3(a["step"]), a["o"], a["d"], a["tmin"], a["tmax"], a["N"], a["dt"], a["t_stop"], f3(a["bg"]),
                                                 a["g"], a["gm"], a["aS"], a["aC"], None)

    def adam(**kw):
        a = dict(sigma=P(sg), coef=P(cf), nx=nx, ny=ny, nz=nz, degree=2, index=P(index), n=na, aS=P(grad.acc_sigma), aC=P(grad.acc_coef), m=P(m),
                 v=P(v), scale=1.0, step=1, lrs=0.1, lrc=0.01, b1=0.9, b2=0.999, eps=1e-8)
        a.update(kw)
        return L.nerf_hip_volume_adam_step(a["sigma"], a["coef"], a["nx"], a["ny"], a["nz"], a["degree"], a["index"], a["n"], a["aS"], a["aC"],
                                           a["m"], a["v"], a["scale"], a["step"], a["lrs"], a["lrc"], a["b1"], a["b2"], a["eps"], None)

    ERR = -1  # NERF_HIP_ERR_ARG
    assert back() == 0 and back(gm=None) == 0 and adam() == 0
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    for kw in [dict(aS=None), dict(aC=None), dict(aS=P(grad.acc_sigma) + 4), dict(aC=P(grad.acc_coef) + 4), dict(g=None), dict(g=P(g) + 2),
               dict(gm=P(gm) + 1), dict(nx=1), dict(degree=3), dict(block=0), dict(dt=0.0), dict(dt=nan), dict(t_stop=1.0), dict(bg=[nan, 0, 0]),
               dict(lo=[inf, 0, 0]), dict(step=[0.0, 1, 1]), dict(N=-1), dict(sigma=None), dict(coef=None), dict(occ=None), dict(o=None),
               dict(d=None), dict(tmin=None), dict(tmax=None)]:
        assert back(**kw) == ERR and L.nerf_hip_last_error(), kw
    assert back(N=0, o=None, d=None, tmin=None, tmax=None, g=None, gm=None) == 0
    for kw in [dict(step=0), dict(step=-3), dict(lrs=nan), dict(lrc=inf), dict(scale=nan), dict(b1=1.0), dict(b2=-0.1), dict(b1=nan), dict(eps=-1.0),
               dict(eps=nan), dict(aS=None), dict(aC=None), dict(aS=P(grad.acc_sigma) + 4), dict(aC=P(grad.acc_coef) + 2), dict(sigma=None),
               dict(coef=None), dict(index=None), dict(m=None), dict(v=None), dict(m=P(m) + 2), dict(n=-1), dict(nz=1), dict(degree=-1)]:
        assert adam(**kw) == ERR and L.nerf_hip_last_error(), kw
    assert adam(n=0, index=None, m=None, v=None) == 0
    torch.cuda.synchronize()
    # the Python layer: an index on the host, accumulators of another type or shape, CPU tensors
    args = (grad.acc_sigma, grad.acc_coef, m, v, 1.0, 1, 0.1, 0.01)
    with pytest.raises(ValueError):
        pkg.ops.volume_adam_step(sg, cf, index.cpu(), *args)
    with pytest.raises(ValueError):
        pkg.ops.volume_adam_step(sg, cf, index, grad.acc_sigma.to(torch.int32), *args[1:])
    with pytest.raises(ValueError):
        pkg.ops.volume_adam_step(sg, cf, index, grad.acc_sigma, grad.acc_coef, m[:, :4].contiguous(), *args[3:])
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.ops.volume_adam_step(sg, cf, index, grad.acc_sigma, grad.acc_coef, m, v, 1.0, 0, 0.1, 0.01)
    with pytest.raises(ValueError):
        pkg.volume.render_backward(vol, pkg.volume.VolumeGrad(grad.acc_sigma.float(), grad.acc_coef), o, d, 0.0, 1.0, g)
    with pytest.raises(RuntimeError):
        pkg.volume.render_backward(vol, grad, o.cpu(), d, 0.0, 1.0, g)
    with pytest.raises(RuntimeError):
        pkg.volume.Finetuner(vol._replace(sigma=vol.sigma.cpu()))
    assert np.array_equal(bits(sg), bits(vol.sigma))                                          # no refused call wrote anything
