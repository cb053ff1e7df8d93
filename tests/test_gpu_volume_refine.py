"""GPU: coarse-to-fine fine-tuning of SH volumes (csrc/volume_refine.hip; rules VM, VT, VX and VP) against the numpy restatements of
tests/volume_refine_reference.py, bit for bit wherever the rule promises it, through volume.Finetuner, its level switch and the
runner; refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import volume_grad_reference as V
import volume_reference as R
import volume_refine_reference as X

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7))
DT = F(0.04)
BG = (0.25, 0.5, 1.0)
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view({4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def scene(shape):
    """the hand-made volume of a lattice (members on the lattice's faces, an empty half) and its active list; computed once"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        index = R.active(sigma)
        _cache[shape] = dict(sigma=sigma, coef=coef, lo=lo, step=step, index=index, member=X.member_mask(index, shape))
    return _cache[shape]


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_volume(pkg, dev, s, block, degree=2, sigma=None, coef=None):
    nc = (degree + 1) ** 2
    sg = on(dev, s["sigma"] if sigma is None else sigma)
    return pkg.volume.Volume(sg, on(dev, (s["coef"] if coef is None else coef)[..., :nc, :]), pkg.volume.blocks(sg, block), s["lo"],
                             s["step"], min(block, pkg.volume.ONE_BLOCK), degree)


def test_member_mask(pkg, dev):
    L = pkg._abi.lib()
    for shape in LATTICES:
        s = scene(shape)
        index = on(dev, s["index"].astype(np.int32))
        vol = device_volume(pkg, dev, s, 2)
        assert np.array_equal(pkg.volume.member_mask(vol, index).cpu().numpy(), s["member"])
        # every byte is written, an index outside the lattice is skipped
        odd = on(dev, np.asarray([0, -1, int(np.prod(shape)), 2**31 - 1, 7], np.int32))
        buf = torch.full(shape, 0xFF, dtype=torch.uint8, device=dev)
        assert L.nerf_hip_volume_member_mask(odd.data_ptr(), 5, *shape, buf.data_ptr(), None) == 0
        assert np.array_equal(buf.cpu().numpy(), X.member_mask([0, 7], shape))
        assert L.nerf_hip_volume_member_mask(None, 0, *shape, buf.data_ptr(), None) == 0 and not buf.any()


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_tv_backward_bits(pkg, dev, shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    vol = device_volume(pkg, dev, s, 2, degree)
    index, member = on(dev, s["index"].astype(np.int32)), on(dev, s["member"])
    rng = np.random.default_rng(3)
    aS = rng.integers(-2 ** 60, 2 ** 60, shape)
    aC = rng.integers(-2 ** 60, 2 ** 60, shape + (nc, 3))
    w, eps = (0.75, 3.0), 1e-9
    want_S, want_C = aS.copy(), aC.copy()
    X.vt(s["sigma"], coef, s["index"], s["member"], w[0], w[1], eps, want_S, want_C)
    assert not np.array_equal(want_S, aS) and not np.array_equal(want_C, aC)
    grad = pkg.volume.VolumeGrad(on(dev, aS), on(dev, aC))
    assert pkg.volume.tv_backward(vol, grad, index, member, w[0], w[1], eps) is grad
    assert np.array_equal(grad.acc_sigma.cpu().numpy(), want_S) and np.array_equal(grad.acc_coef.cpu().numpy(), want_C)
    # chunks that cover the list once, in any order, with the mask of the whole list
    grad2 = pkg.volume.VolumeGrad(on(dev, aS), on(dev, aC))
    n = int(index.shape[0])
    for a, b in ((n // 2, n), (0, 3), (3, n // 2)):
        pkg.volume.tv_backward(vol, grad2, index[a:b], member, w[0], w[1], eps)
    assert np.array_equal(grad2.acc_sigma.cpu().numpy(), want_S) and np.array_equal(grad2.acc_coef.cpu().numpy(), want_C)
    assert np.array_equal(bits(vol.sigma), bits(s["sigma"])) and np.array_equal(bits(vol.coef), bits(coef))


@pytest.mark.parametrize("shape", LATTICES)
def test_tv_backward_invariants(pkg, dev, shape):
    s = scene(shape)
    vol = device_volume(pkg, dev, s, 2)
    index, member = on(dev, s["index"].astype(np.int32)), on(dev, s["member"])
    outside = s["member"].reshape(-1) == 0
    assert outside.any()
    grad = pkg.volume.tv_backward(vol, pkg.volume.grad_buffers(vol), index, member, 2.0, 0.5)
    gS, gC = grad.acc_sigma.cpu().numpy().reshape(-1), grad.acc_coef.cpu().numpy().reshape(-1, 27)
    assert gS.any() and gC.any() and not gS[outside].any() and not gC[outside].any()
    assert gS.sum() == 0 and not gC.sum(0).any()                       # per word type: exactly 0 (int64 sums)
    # the default eps is 1e-9
    want_S, want_C = np.zeros(shape, np.int64), np.zeros(shape + (9, 3), np.int64)
    X.vt(s["sigma"], s["coef"], s["index"], s["member"], 2.0, 0.5, 1e-9, want_S, want_C)
    assert np.array_equal(gS, want_S.reshape(-1)) and np.array_equal(gC, want_C.reshape(-1, 27))
    # one weight 0: that word type is untouched; both 0: nothing is
    rng = np.random.default_rng(1)
    aS, aC = rng.integers(-2 ** 40, 2 ** 40, shape), rng.integers(-2 ** 40, 2 ** 40, shape + (9, 3))
    g = pkg.volume.tv_backward(vol, pkg.volume.VolumeGrad(on(dev, aS), on(dev, aC)), index, member, 0.0, 0.0)
    assert np.array_equal(g.acc_sigma.cpu().numpy(), aS) and np.array_equal(g.acc_coef.cpu().numpy(), aC)
    g = pkg.volume.tv_backward(vol, g, index, member, 0.0, 1.0)
    assert np.array_equal(g.acc_sigma.cpu().numpy(), aS) and not np.array_equal(g.acc_coef.cpu().numpy(), aC)
    # a list entry that is not in the mask, or outside the lattice, receives nothing
    stray = on(dev, np.asarray([int(np.flatnonzero(outside)[0]), -5, int(np.prod(shape))], np.int32))
    g = pkg.volume.tv_backward(vol, pkg.volume.VolumeGrad(on(dev, aS), on(dev, aC)), stray, member, 1.0, 1.0)
    assert np.array_equal(g.acc_sigma.cpu().numpy(), aS) and np.array_equal(g.acc_coef.cpu().numpy(), aC)


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_upsample_and_prune_bits(pkg, dev, shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    sigma = s["sigma"].copy()
    sigma[2, 1, 1], sigma[3, 1, 1] = -1.0, -0.0
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    vol = device_volume(pkg, dev, s, 2, degree, sigma=sigma)
    up = pkg.volume.upsample(vol)
    s2, c2 = X.vx(sigma, coef)
    assert tuple(up.sigma.shape) == X.up_shape(shape) == {(5, 4, 3): (9, 7, 5), (9, 8, 7): (17, 15, 13)}[shape]
    assert np.array_equal(bits(up.sigma), bits(s2)) and np.array_equal(bits(up.coef), bits(c2))
    assert np.array_equal(up.lo, s["lo"]) and np.array_equal(up.step, X.half_step(s["step"])) and (up.block, up.degree) == (2, degree)
    assert np.array_equal(up.occ.cpu().numpy(), pkg.volume.blocks(up.sigma, 2).cpu().numpy())
    assert np.array_equal(up.occ.cpu().numpy(), R.blocks(s2, 2))
    assert np.array_equal(bits(vol.sigma), bits(sigma)) and np.array_equal(bits(vol.coef), bits(coef))
    sigma = sigma.copy()
    sigma[1, 1, 1] = np.nan                                       # (not refined: a NaN's payload is not the rule's business)
    vol = device_volume(pkg, dev, s, 2, degree, sigma=sigma)
    for thr in (0.0, 3.0):
        pr = pkg.volume.prune(vol, thr)
        ws, wc = X.vp(sigma, coef, thr)
        assert np.array_equal(bits(pr.sigma), bits(ws)) and np.array_equal(bits(pr.coef), bits(wc))
        assert np.array_equal(pr.occ.cpu().numpy(), R.blocks(ws, 2)) and (pr.block, pr.degree) == (2, degree)
        assert not np.isnan(ws).any() and (wc != coef).any()
    assert np.array_equal(bits(vol.sigma), bits(sigma)) and np.array_equal(bits(vol.coef), bits(coef))      # the inputs keep their bits


@pytest.mark.parametrize("shape", LATTICES)
def test_refined_render(pkg, dev, shape):
    """The refined volume renders what the coarse one does, within a bound derived from the lookup bound of
    volume_refine_reference: with t_stop = 0 a ray's colour is C = sum_i w_i c_i + (1 - A) bg over its samples.  A lookup moves a
    sample's sigma_s (taken as 0 where it is not > 0) by at most b_s and its colour by at most b_c.  d C / d sigma_j =
    dt (T_(j+1) c_j - sum_(i>j) w_i c_i) is a difference of two numbers in [0, 1], so |d C / d sigma_j| <= dt, the same for A; and
    sum_i w_i <= 1.  With n the samples that contribute in either render (at most n_coarse + n_fine):
        |rgb' - rgb| <= (1 + max |bg|) n dt b_s + b_c + the two fp32 marches' own roundings, 2 R.bound(n) (1 + max |bg|)."""
    s = scene(shape)
    vol = device_volume(pkg, dev, s, 2)
    up = pkg.volume.upsample(vol)
    o, d, tmin, tmax = R.make_rays(300, 5, s["lo"], s["step"], shape)
    rays = tuple(on(dev, a) for a in (o, d, tmin, tmax))
    a = [t.cpu().numpy() for t in pkg.volume.render(vol, *rays, dt=DT, t_stop=0.0, background=BG)]
    b = [t.cpu().numpy() for t in pkg.volume.render(up, *rays, dt=DT, t_stop=0.0, background=BG)]
    bs, bc = X.lookup_bounds(s["sigma"], s["coef"], d)
    n = (a[2][:, 0] + b[2][:, 0]).astype(np.float64)
    bound = 2.0 * n * float(DT) * bs + bc + 2 * R.bound(n) * 2.0
    hit = a[2][:, 0] > 0
    err = np.abs(a[0].astype(np.float64) - b[0]).max(1)
    print("refined render: worst |rgb' - rgb| / bound", float((err[hit] / bound[hit]).max()), "worst", float(err.max()))
    assert hit.sum() > 100 and (err <= bound).all()
    # the block edge plays no role in the refined render
    for B in (1, 3, pkg.volume.ONE_BLOCK):
        c = pkg.volume.render(pkg.volume.with_block(up, B), *rays, dt=DT, t_stop=0.0, background=BG)
        assert np.array_equal(bits(c[0]), bits(b[0])) and np.array_equal(bits(c[1]), bits(b[1]))
        assert np.array_equal(c[2][:, 0].cpu().numpy(), b[2][:, 0])


def learning_volume(pkg, dev, case):
    sigma = on(dev, case["s2"])
    return pkg.volume.Volume(sigma, on(dev, case["c2"]), pkg.volume.blocks(sigma, 2), case["lo"], case["step"], 2, 2)


def test_finetuner_composition(pkg, dev):
    case = V.learning_case()
    vol = learning_volume(pkg, dev, case)
    rays = tuple(on(dev, case[k]) for k in ("o", "d", "tmin", "tmax"))
    target = on(dev, case["target"])
    kw = dict(background=V.LEARN_BG, dt=V.LEARN_DT, t_stop=0.0)
    # weights 0: the plain tuner, bit for bit, and no mask
    plain, zero = pkg.volume.Finetuner(vol), pkg.volume.Finetuner(vol, tv_sigma=0.0, tv_coef=0.0, tv_eps=1e-9)
    assert zero.member is None
    for _ in range(3):
        la, lb = plain.step(*rays, target, **kw), zero.step(*rays, target, **kw)
        assert np.array_equal(bits(la), bits(lb))
    for name in ("m", "v"):
        assert np.array_equal(bits(getattr(plain, name)), bits(getattr(zero, name)))
    assert np.array_equal(bits(plain.vol.sigma), bits(zero.vol.sigma)) and np.array_equal(bits(plain.vol.coef), bits(zero.vol.coef))
    # weights > 0: one step is render + render_backward + tv_backward + the Adam step through the public calls
    tv = (2e-3, 1e-3)
    tuner = pkg.volume.Finetuner(vol, tv_sigma=tv[0], tv_coef=tv[1])
    assert np.array_equal(tuner.member.cpu().numpy(), X.member_mask(case["index"], case["s2"].shape))
    loss = tuner.step(*rays, target, **kw)
    work = vol._replace(sigma=vol.sigma.clone(), coef=vol.coef.clone())
    index = pkg.volume.active(vol.sigma)
    n, N = int(index.shape[0]), int(rays[0].shape[0])
    rgb = pkg.volume.render(work, *rays, **kw)[0]
    diff = rgb - target
    grad = pkg.volume.render_backward(work, pkg.volume.grad_buffers(work), *rays, 2.0 * diff, None, **kw)
    pkg.volume.tv_backward(work, grad, index, pkg.volume.member_mask(work, index), tv[0] / n * 3 * N, tv[1] / n * 3 * N, 1e-9)
    m, v = torch.zeros(n, 28, device=dev), torch.zeros(n, 28, device=dev)
    pkg.ops.volume_adam_step(work.sigma, work.coef, index, grad.acc_sigma, grad.acc_coef, m, v, 1.0 / (3.0 * N), 1, 0.1, 0.01)
    assert np.array_equal(bits(loss), bits((diff * diff).mean()))
    for got, want in ((tuner.vol.sigma, work.sigma), (tuner.vol.coef, work.coef), (tuner.m, m), (tuner.v, v)):
        assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(tuner.vol.coef), bits(plain.vol.coef)) and not tuner.grad.acc_sigma.any() and not tuner.grad.acc_coef.any()
    assert np.array_equal(bits(vol.sigma), bits(case["s2"]))


@pytest.mark.parametrize("tv", (0.0, 1e-3))
def test_finetune_schedule(pkg, dev, tv):
    """learning_case through Finetuner levels (finetune's own level switch, Finetuner.refined): 25 full-batch steps at the default
    rates, the lattice doubled after step 12.  The factor 2 against the restatement's own final loss is the existing learning test's
    allowance for fp32-vs-fp64 forward and quantised sums; it is not a measured margin."""
    case = V.learning_case()
    want = X.learn_levels(case, upsample_at=(12,), tv=(tv, tv))["losses"]
    vol = learning_volume(pkg, dev, case)
    rays = tuple(on(dev, case[k]) for k in ("o", "d", "tmin", "tmax"))
    target = on(dev, case["target"])
    kw = dict(background=V.LEARN_BG, dt=V.LEARN_DT, t_stop=0.0)
    tuner = pkg.volume.Finetuner(vol, tv_sigma=tv, tv_coef=tv)
    losses, levels = [], [(tuner, tuner.vol.sigma.clone())]
    for it in range(V.LEARN_STEPS):
        if it == 12:
            old = tuner
            tuner = old.refined(None)
            assert old.m is None and old.grad is None and tuner.steps == 0 and not tuner.m.any()
            assert (tuner.lr_sigma, tuner.lr_coef, tuner.tv_sigma, tuner.tv_coef) == (old.lr_sigma, old.lr_coef, tv, tv)
            levels.append((tuner, tuner.vol.sigma.clone()))
        losses.append(tuner.step(*rays, target, **kw))
    out = tuner.volume()
    assert len(losses) == 25 and tuner.steps == 13
    final = float(((pkg.volume.render(out, *rays, **kw)[0] - target) ** 2).mean())
    first = float(losses[0])
    print(f"tv={tv}: loss {first:.3e} -> {final:.3e} ({final / first:.4f}); the restatement: {want[0]:.3e} -> {want[-1]:.3e}; "
          f"across the switch {float(losses[11]):.4e} {float(losses[12]):.4e}")
    assert final <= 2.0 * want[-1] and final <= 0.25 * first
    assert tuple(out.sigma.shape) == (17, 15, 13) and np.array_equal(out.step, X.half_step(case["step"])) and np.array_equal(out.lo, case["lo"])
    assert np.array_equal(out.occ.cpu().numpy(), R.blocks(out.sigma.cpu().numpy(), 2)) and (out.block, out.degree) == (2, 2)
    # the frozen support, level by level: outside a level's list nothing moved, a zero sigma stayed zero, the accumulators are clean
    for t, start in levels:
        outside = torch.ones(start.numel(), dtype=torch.bool, device=dev)
        outside[t.index.long()] = False
        assert np.array_equal(bits(t.vol.sigma.reshape(-1)[outside]), bits(start.reshape(-1)[outside]))
        assert not (t.vol.sigma[start == 0] != 0).any()
    assert not tuner.grad.acc_sigma.any() and not tuner.grad.acc_coef.any()
    assert np.array_equal(tuner.index.cpu().numpy(), R.active(levels[1][1].cpu().numpy()))


def test_runner_coarse_to_fine(pkg, dev, tmp_path, capsys):
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    rs = str(tmp_path) + "/rs/"
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=20, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=20)
    run.trainer("train")
    capsys.readouterr()
    vol = run.bake_volume(16, degree=1, finetune=6, finetune_batch=128, finetune_upsample=(3,), finetune_tv=(1e-3, 1e-3), finetune_prune=0.0)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[VOLUME]")]
    assert len(lines) == 2 and "finetune 6 steps" in lines[1] and "31x31x31" in lines[1] and "TV" in lines[1] and "loss" in lines[1]
    tuned = glob.glob(rs + "*_ft*.npz")
    assert len(tuned) == 1 and os.path.basename(tuned[0]) == f"{run.start_time}_{run.last_iter}_volume16_ft6_up1.npz"
    back = pkg.volume.load(tuned[0], dev)
    assert tuple(back.sigma.shape) == (31, 31, 31) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(back[:3], vol[:3]))
    assert np.array_equal(back.step * F(2), pkg.volume.load(glob.glob(rs + "*_volume16.npz")[0], dev).step)
    ft = run.last_volume_finetune
    assert ft["iters"] == 6 and ft["shape"] == (31, 31, 31) and np.isfinite(ft["last_loss"])
    # without the new arguments: today's names and lines
    run.bake_volume(16, degree=1, finetune=2, finetune_batch=128)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[VOLUME]")]
    assert len(lines) == 2 and "TV" not in lines[1] and "upsample" not in lines[1] and "2 steps of 128 train rays: batch loss" in lines[1]
    assert len(glob.glob(rs + "*_volume16_ft2.npz")) == 1 and len(glob.glob(rs + "*_up*.npz")) == 1
    assert run.last_volume_finetune["shape"] == (16, 16, 16)
    # schedule errors come before any work
    for kw in (dict(finetune_upsample=(6,)), dict(finetune_upsample=(0,)), dict(finetune_upsample=(3, 3)), dict(finetune_upsample=(4, 2)),
               dict(finetune_prune=-1.0), dict(finetune_prune=float("nan")), dict(finetune_tv=(-1.0, 0.0)), dict(finetune_tv=(1.0,))):
        with pytest.raises(ValueError):
            run.bake_volume(16, degree=1, finetune=6, finetune_batch=128, save=False, **kw)
    with pytest.raises(ValueError):
        run.bake_volume(16, degree=1, finetune_upsample=(3,))
    assert capsys.readouterr().out.count("[VOLUME]") == 0


def test_refusals(pkg, dev):
    L = pkg._abi.lib()
    s = scene((5, 4, 3))
    vol = device_volume(pkg, dev, s, 2)
    nx, ny, nz = 5, 4, 3
    index = on(dev, s["index"].astype(np.int32))
    member = on(dev, s["member"])
    na = int(index.shape[0])
    grad = pkg.volume.grad_buffers(vol)
    sg, cf = vol.sigma.clone(), vol.coef.clone()
    s2, c2 = torch.zeros(9, 7, 5, device=dev), torch.zeros(9, 7, 5, 9, 3, device=dev)
    mbuf = torch.zeros(5, 4, 3, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()

    def mask(**kw):
        a = dict(index=P(index), n=na, nx=nx, ny=ny, nz=nz, member=P(mbuf))
        a.update(kw)
        return L.nerf_hip_volume_member_mask(a["index"], a["n"], a["nx"], a["ny"], a["nz"], a["member"], None)

    def tv(**kw):
        a = dict(sigma=P(sg), coef=P(cf), nx=nx, ny=ny, nz=nz, degree=2, index=P(index), n=na, member=P(member), ws=1.0, wc=1.0, eps=1e-9,
                 aS=P(grad.acc_sigma), aC=P(grad.acc_coef))
        a.update(kw)
        return L.nerf_hip_volume_tv_backward(a["sigma"], a["coef"], a["nx"], a["ny"], a["nz"], a["degree"], a["index"], a["n"], a["member"],
                                             a["ws"], a["wc"], a["eps"], a["aS"], a["aC"], None)

    def up(**kw):
        a = dict(sigma=P(sg), coef=P(cf), nx=nx, ny=ny, nz=nz, degree=2, s2=P(s2), c2=P(c2))
        a.update(kw)
        return L.nerf_hip_volume_upsample(a["sigma"], a["coef"], a["nx"], a["ny"], a["nz"], a["degree"], a["s2"], a["c2"], None)

    def prune(**kw):
        a = dict(sigma=P(sg), coef=P(cf), nx=nx, ny=ny, nz=nz, degree=2, thr=0.0)
        a.update(kw)
        return L.nerf_hip_volume_prune(a["sigma"], a["coef"], a["nx"], a["ny"], a["nz"], a["degree"], a["thr"], None)

    ERR = -1  # NERF_HIP_ERR_ARG
    nan, inf = float("nan"), float("inf")
    for kw in [dict(index=None), dict(index=P(index) + 2), dict(member=None), dict(n=-1), dict(n=2**31), dict(nx=1), dict(nz=0)]:
        assert mask(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in [dict(eps=0.0), dict(eps=-1.0), dict(eps=nan), dict(eps=inf), dict(ws=-1.0), dict(wc=-1e-3), dict(ws=nan), dict(wc=inf),
               dict(ws=65537.0), dict(wc=1e9), dict(sigma=None), dict(coef=None), dict(sigma=P(sg) + 2), dict(coef=P(cf) + 1), dict(index=None),
               dict(index=P(index) + 2), dict(member=None), dict(aS=None), dict(aC=None), dict(aS=P(grad.acc_sigma) + 4),
               dict(aC=P(grad.acc_coef) + 4), dict(n=-1), dict(n=2**31), dict(ny=1), dict(degree=3), dict(degree=-1)]:
        assert tv(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in [dict(sigma=None), dict(coef=None), dict(s2=None), dict(c2=None), dict(s2=P(s2) + 2), dict(c2=P(c2) + 1), dict(nx=1), dict(degree=3),
               dict(nx=1025, ny=1025, nz=1025), dict(nx=2**30, ny=2, nz=2), dict(nx=32768, ny=32768, nz=2)]:
        assert up(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in [dict(thr=-1.0), dict(thr=nan), dict(thr=inf), dict(sigma=None), dict(coef=None), dict(sigma=P(sg) + 2), dict(nz=1), dict(degree=3)]:
        assert prune(**kw) == ERR and L.nerf_hip_last_error(), kw
    torch.cuda.synchronize()
    # no refused call wrote anything
    assert not grad.acc_sigma.any() and not grad.acc_coef.any() and not s2.any() and not c2.any() and not mbuf.any()
    assert np.array_equal(bits(sg), bits(vol.sigma)) and np.array_equal(bits(cf), bits(vol.coef))
    # counts of 0, and both weights 0, succeed
    assert mask(n=0, index=None) == 0 and tv(n=0, index=None) == 0 and tv(ws=0.0, wc=0.0, index=None) == 0
    assert mask() == 0 and tv() == 0 and up() == 0 and prune() == 0
    torch.cuda.synchronize()
    assert grad.acc_sigma.any() and s2.any() and mbuf.any()
    # the Python layer
    with pytest.raises(ValueError):
        pkg.ops.volume_member_mask(index.cpu(), (5, 4, 3))
    with pytest.raises(ValueError):
        pkg.volume.tv_backward(vol, grad, index, member.to(torch.int32), 1.0, 1.0)
    with pytest.raises(ValueError):
        pkg.volume.tv_backward(vol, grad, index, member[:4].contiguous(), 1.0, 1.0)
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.volume.tv_backward(vol, grad, index, member, 1.0, 1.0, eps=0.0)
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.volume.prune(vol, -1.0)
    with pytest.raises(RuntimeError):
        pkg.volume.upsample(vol._replace(sigma=vol.sigma.cpu()))
    with pytest.raises(ValueError):
        pkg.volume.Finetuner(vol, tv_sigma=-1.0)
    with pytest.raises(ValueError):
        pkg.volume.Finetuner(vol, tv_coef=1.0, tv_eps=0.0)
    for bad in (dict(upsample_at=(5,)), dict(upsample_at=(0,)), dict(upsample_at=(2, 2)), dict(upsample_at=(3, 1)), dict(upsample_at=(1.5,)),
                dict(upsample_at=(1,), prune=-1.0), dict(upsample_at=(1,), tv_sigma=float("nan"))):
        with pytest.raises(ValueError):                             # before any step: the rays are never looked at
            pkg.volume.finetune(vol, None, None, 5, **bad)
    with pytest.raises(ValueError):                                 # the 2^31 limit at the last level: 300 -> 599 -> 1197 -> 2393
        pkg.volume.check_schedule((300, 300, 300), 9, (1, 2, 3))
    assert pkg.volume.check_schedule((300, 300, 300), 9, (1, 2))[1] == (1197, 1197, 1197)
    assert pkg.volume.check_schedule((16, 16, 16), 6, (3,), 0.0) == ((3,), (31, 31, 31))
