"""GPU: fine-tuning compact SH radiance volumes (csrc/volume_compact_grad.hip; rules VCG, VCU and VCT of include/nerf_hip.h) -- every
compact training call against the DENSE kernel on the same device, gathered at the rows, bit for bit (garbage at the dense volume's
inactive points included: tests/test_volume_compact_train_cpu.py shows on the restatements that it adds nothing outside the list), the
update also against the numpy restatement, the tuner and the schedule against Finetuner / finetune on the unpacked volume, a memory
condition, the runner, refusals."""
import glob
import os

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_compact_train_reference as T
import volume_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))   # 27 / 130 / 324 rows: one partial workgroup .. several
BLOCKS = (1, 2, 4, 8, 1 << 30)                   # the last: one block
NRAYS = 300
DT = F(0.04)
BG = (0.25, 0.5, 1.0)
_cache = {}


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)


def bits(a):
    a = host(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def scene(shape):
    """make_volume with garbage sigma at its inactive points (the coefficients are random everywhere), the rays and upstream values"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        garbage, inactive = X.with_garbage(sigma, coef)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        rng = np.random.default_rng(7)
        _cache[shape] = dict(sigma=garbage, inactive=inactive, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax,
                             g_rgb=rng.normal(0.0, 1.0, (NRAYS, 3)).astype(F), g_maps=rng.normal(0.0, 1.0, (NRAYS, 2)).astype(F),
                             index=R.active(garbage))
    return _cache[shape]


def device_volume(pkg, dev, s, block=2, degree=2):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sg = t(s["sigma"])
    return pkg.volume.Volume(sg, t(s["coef"][..., :(degree + 1) ** 2, :]), pkg.volume.blocks(sg, block), s["lo"], s["step"],
                             min(block, pkg.volume.ONE_BLOCK), degree)


def rays_on(dev, s, sel=slice(None)):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    return t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"])


def backward(pkg, dev, s, vol, sel=slice(None), grad=None, t_stop=0.0, maps=True, g_rgb=None):
    """render_backward / compact_render_backward of the scene's rays ``sel`` into ``grad`` (fresh buffers when None)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    compact = isinstance(vol, pkg.volume.CompactVolume)
    if grad is None:
        grad = pkg.volume.compact_grad_buffers(vol) if compact else pkg.volume.grad_buffers(vol)
    call = pkg.volume.compact_render_backward if compact else pkg.volume.render_backward
    return call(vol, grad, *rays_on(dev, s, sel), t(s["g_rgb"] if g_rgb is None else g_rgb), t(s["g_maps"]) if maps else None, dt=DT,
                t_stop=t_stop, background=BG)


def gathered(dense_grad, index, dev):
    """the dense accumulators at the lattice points index -> ([n], [n, 3 nc]) and whether everything else is 0"""
    idx = torch.as_tensor(np.asarray(index, np.int64), device=dev)
    aS, aC = dense_grad.acc_sigma.reshape(-1), dense_grad.acc_coef.reshape(dense_grad.acc_sigma.numel(), -1)
    outside = torch.ones(aS.numel(), dtype=torch.bool, device=dev)
    outside[idx] = False
    return aS[idx], aC[idx], not aS[outside].any() and not aC[outside].any()


def equal_at_rows(cgrad, dgrad, index, dev):
    gS, gC, clean = gathered(dgrad, index, dev)
    return clean and same(cgrad.acc_sigma, gS) and same(cgrad.acc_coef, gC)


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_backward_equals_dense(pkg, dev, shape, degree):
    s = scene(shape)
    index = s["index"]
    hits = 0
    for B in BLOCKS:
        dv = device_volume(pkg, dev, s, B, degree)                                 # the garbage is there
        cv = pkg.volume.pack(dv)
        assert torch.isnan(dv.sigma).any() and cv.sigma.shape[0] == (27, 130, 324)[LATTICES.index(shape)]
        assert same(pkg.volume.row_points(cv), index.astype(np.int32))
        for t_stop in (0.0, 0.3):
            for maps in (True, False):
                dg = backward(pkg, dev, s, dv, t_stop=t_stop, maps=maps)
                cg = backward(pkg, dev, s, cv, t_stop=t_stop, maps=maps)
                assert isinstance(cg, pkg.volume.CompactGrad) and cg.acc_coef.shape == (len(index), 3 * (degree + 1) ** 2)
                assert equal_at_rows(cg, dg, index, dev), (B, t_stop, maps)
                hits += int(cg.acc_sigma.count_nonzero()) + int(cg.acc_coef.count_nonzero())
                if B == 2:
                    for n in (0, 1, 130):
                        sel = slice(0, n) if n != 1 else slice(7, 8)
                        assert equal_at_rows(backward(pkg, dev, s, cv, sel=sel, t_stop=t_stop, maps=maps),
                                             backward(pkg, dev, s, dv, sel=sel, t_stop=t_stop, maps=maps), index, dev), (n, t_stop, maps)
    assert hits > 20 * len(index)                                                  # the equalities are not over zeros
    # gradients() reads the rows' accumulators as it reads the dense ones
    d_sigma, d_coef = pkg.volume.gradients(cg, scale=0.5)
    assert same(d_sigma, (host(cg.acc_sigma).astype(np.float64) * 2.0 ** -40 * 0.5).astype(F))
    assert d_coef.shape == cg.acc_coef.shape and d_coef.dtype == torch.float32


@pytest.mark.parametrize("shape", LATTICES)
def test_order_independence(pkg, dev, shape):
    s = scene(shape)
    cv = pkg.volume.pack(device_volume(pkg, dev, s, 2))
    base = backward(pkg, dev, s, cv, t_stop=0.3)
    eq = lambda g: same(g.acc_sigma, base.acc_sigma) and same(g.acc_coef, base.acc_coef)
    assert base.acc_sigma.any() and base.acc_coef.any()
    assert eq(backward(pkg, dev, s, cv, t_stop=0.3))                               # the same call twice
    perm = np.random.default_rng(1).permutation(NRAYS)
    assert eq(backward(pkg, dev, s, cv, sel=perm, t_stop=0.3))                     # the rays permuted
    two = backward(pkg, dev, s, cv, sel=slice(0, 130), t_stop=0.3)
    assert not eq(two)
    assert eq(backward(pkg, dev, s, cv, sel=slice(130, NRAYS), grad=two, t_stop=0.3))          # a batch split into two accumulating calls


def test_zero_and_unusual_inputs(pkg, dev):
    shape = (9, 8, 7)
    s = scene(shape)
    index = s["index"]
    dv = device_volume(pkg, dev, s, 2)
    cv = pkg.volume.pack(dv)
    n = int(cv.sigma.shape[0])
    none = lambda g: not g.acc_sigma.any() and not g.acc_coef.any()
    # a slot lattice that lacks one corner of contributing cells: that corner receives nothing, the other rows equal the dense gather
    whole = backward(pkg, dev, s, cv)
    positive = host(cv.sigma) > 0
    r = int(np.flatnonzero((host(whole.acc_sigma) != 0) & ~positive)[0])           # a corner that contributes only as a neighbour
    for bad_slot in (-1, n, -2):
        slot = cv.slot.clone()
        slot.view(-1)[int(index[r])] = bad_slot
        bad = cv._replace(slot=slot)
        ub = pkg.volume.unpack(bad)                                                # +0 at that point: the dense volume of the claim
        cg, dg = backward(pkg, dev, s, bad), backward(pkg, dev, s, ub)
        gS, gC, clean = gathered(dg, index, dev)
        keep = torch.arange(n, device=dev) != r
        assert clean and gS[r] != 0 and gC[r].any()                                # the dense kernel does add at that point
        assert cg.acc_sigma[r] == 0 and not cg.acc_coef[r].any()
        assert same(cg.acc_sigma[keep], gS[keep]) and same(cg.acc_coef[keep], gC[keep]) and cg.acc_sigma.any()
    # no rows at all
    nothing = np.zeros(shape, F)
    nothing[1, 1, 1], nothing[0, 0, 0] = np.nan, -1.0
    c0 = pkg.volume.pack(device_volume(pkg, dev, {**s, "sigma": nothing}, 2))
    g0 = backward(pkg, dev, s, c0)
    assert c0.sigma.shape == (0,) and g0.acc_sigma.shape == (0,) and g0.acc_coef.shape == (0, 27)
    # no rays, rays that all miss
    assert none(backward(pkg, dev, s, cv, sel=slice(0, 0)))
    steps = host(pkg.volume.render(cv, *rays_on(dev, s), dt=DT, t_stop=0.0, background=BG)[2])
    miss = np.flatnonzero(steps[:, 1] == 0)
    assert miss.size >= NRAYS // 10 and none(backward(pkg, dev, s, cv, sel=miss))
    # a NaN (or inf) upstream value silences its ray, and only its ray
    r = int(np.flatnonzero(steps[:, 0] >= 3)[0])
    for bad, ch in ((np.nan, 1), (np.inf, 2)):
        g = s["g_rgb"].copy()
        g[r, ch] = bad
        assert none(backward(pkg, dev, s, cv, sel=slice(r, r + 1), g_rgb=g))
        rest = np.delete(np.arange(NRAYS), r)
        a, b = backward(pkg, dev, s, cv, g_rgb=g), backward(pkg, dev, s, cv, sel=rest)
        assert same(a.acc_sigma, b.acc_sigma) and same(a.acc_coef, b.acc_coef) and not none(a)
    gm = {**s, "g_maps": s["g_maps"].copy()}
    gm["g_maps"][r, 0] = np.nan
    assert none(backward(pkg, dev, gm, cv, sel=slice(r, r + 1))) and not none(backward(pkg, dev, s, cv, sel=slice(r, r + 1)))


@pytest.mark.parametrize("degree", (0, 1, 2))
def test_update(pkg, dev, degree):
    """three Adam steps after real backward calls, at a rate of 3 per step so that rows die: the rows against the device's dense step
    on the unpacked volume and against the numpy restatement"""
    shape = (9, 8, 7)
    s = scene(shape)
    index = s["index"]
    nc = (degree + 1) ** 2
    cv = pkg.volume.pack(device_volume(pkg, dev, s, 2, degree))
    n, words = len(index), 1 + 3 * nc
    start = cv.sigma.clone()
    c_sigma, c_coef = cv.sigma.clone(), cv.coef.clone()
    dense = pkg.volume.unpack(cv)
    d_index = torch.from_numpy(index.astype(np.int32)).to(dev)
    c_m, c_v, d_m, d_v = (torch.zeros(n, words, device=dev) for _ in range(4))
    h_sigma, h_coef, h_m, h_v = host(c_sigma).copy(), host(c_coef).copy(), np.zeros((n, words), F), np.zeros((n, words), F)
    cg, dg = pkg.volume.compact_grad_buffers(cv), pkg.volume.grad_buffers(dense)
    for step in (1, 2, 3):
        work = cv._replace(sigma=c_sigma, coef=c_coef)
        backward(pkg, dev, s, work, grad=cg, t_stop=0.3)
        backward(pkg, dev, s, dense, grad=dg, t_stop=0.3)
        assert equal_at_rows(cg, dg, index, dev) and cg.acc_sigma.any(), step
        h_aS, h_aC = host(cg.acc_sigma).copy(), host(cg.acc_coef).copy()
        pkg.ops.volume_compact_adam_step(c_sigma, c_coef, degree, cg.acc_sigma, cg.acc_coef, c_m, c_v, 1.0 / (3 * NRAYS), step, 3.0, 0.01)
        pkg.ops.volume_adam_step(dense.sigma, dense.coef, d_index, dg.acc_sigma, dg.acc_coef, d_m, d_v, 1.0 / (3 * NRAYS), step, 3.0, 0.01)
        T.vcu_step(h_sigma, h_coef, h_aS, h_aC, h_m, h_v, 1.0 / (3 * NRAYS), step, 3.0, 0.01)
        assert not cg.acc_sigma.any() and not cg.acc_coef.any() and not dg.acc_sigma.any() and not dg.acc_coef.any()
        gS, gC, _ = gathered(pkg.volume.VolumeGrad(dense.sigma, dense.coef), index, dev)
        for got, dev_dense, restated in ((c_sigma, gS, h_sigma), (c_coef, gC, h_coef), (c_m, d_m, h_m), (c_v, d_v, h_v)):
            assert same(got, dev_dense) and same(got, restated), step
        if step == 2:
            died = (c_sigma == 0) & (start > 0)
    assert died.any() and not (c_sigma[died] != 0).any()                           # a row died on the way, and stayed dead
    assert (c_sigma > 0).any() and same(cv.sigma, start)                           # the input was not touched


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_tv(pkg, dev, shape, degree):
    s = scene(shape)
    index = s["index"]
    cv = pkg.volume.pack(device_volume(pkg, dev, s, 2, degree))
    dense = pkg.volume.unpack(cv)
    d_index = pkg.volume.row_points(cv)
    member = pkg.volume.member_mask(dense, d_index)
    for w_sigma, w_coef in ((0.7, 0.3), (0.0, 2.0), (3.0, 0.0), (0.0, 0.0)):
        cg = pkg.volume.compact_tv_backward(cv, pkg.volume.compact_grad_buffers(cv), w_sigma, w_coef)
        dg = pkg.volume.tv_backward(dense, pkg.volume.grad_buffers(dense), d_index, member, w_sigma, w_coef)
        assert equal_at_rows(cg, dg, index, dev), (w_sigma, w_coef)
        assert int(cg.acc_sigma.sum()) == 0 and not cg.acc_coef.sum(0).any()       # each word type's integers sum to exactly 0
        assert bool(cg.acc_sigma.any()) == (w_sigma > 0) and bool(cg.acc_coef.any()) == (w_coef > 0)
    # the terms are ADDED to what the accumulators hold
    both = backward(pkg, dev, s, cv)
    march = (both.acc_sigma.clone(), both.acc_coef.clone())
    pkg.volume.compact_tv_backward(cv, both, 0.7, 0.3)
    tv = pkg.volume.compact_tv_backward(cv, pkg.volume.compact_grad_buffers(cv), 0.7, 0.3)
    assert same(both.acc_sigma, march[0] + tv.acc_sigma) and same(both.acc_coef, march[1] + tv.acc_coef)
    n = len(index)
    # a point list that disagrees with the slots: the rows whose point names another row receive nothing, the others what they did
    swapped = d_index.clone()
    swapped[[1, n - 2]] = d_index[[n - 2, 1]]
    sw = pkg.volume.compact_grad_buffers(cv)
    pkg.ops.volume_compact_tv_backward(cv.slot, cv.sigma, cv.coef, cv.degree, swapped, 0.7, 0.3, 1e-9, sw.acc_sigma, sw.acc_coef)
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[[1, n - 2]] = False
    assert not sw.acc_sigma[~keep].any() and not sw.acc_coef[~keep].any() and tv.acc_coef[~keep].any()
    assert same(sw.acc_sigma[keep], tv.acc_sigma[keep]) and same(sw.acc_coef[keep], tv.acc_coef[keep])
    # a slot outside [0, n) is no member: its row receives nothing, its neighbours see a constant there
    slot = cv.slot.clone()
    pts = index[[n // 3, 2 * n // 3]]
    slot.view(-1)[int(pts[0])], slot.view(-1)[int(pts[1])] = n, -2
    bad = cv._replace(slot=slot)
    cg = pkg.volume.compact_tv_backward(bad, pkg.volume.compact_grad_buffers(bad), 0.7, 0.3)
    ub = pkg.volume.unpack(bad)
    rest = torch.from_numpy(np.setdiff1d(index, pts).astype(np.int32)).to(dev)
    dg = pkg.volume.tv_backward(ub, pkg.volume.grad_buffers(ub), rest, pkg.volume.member_mask(ub, rest), 0.7, 0.3)
    assert equal_at_rows(cg, dg, index, dev) and not cg.acc_sigma[[n // 3, 2 * n // 3]].any() and cg.acc_sigma.any()


def same_compact(a, b):
    return (same(a.slot, b.slot) and same(a.sigma, b.sigma) and same(a.coef, b.coef) and same(a.occ, b.occ) and np.array_equal(a.lo, b.lo)
            and np.array_equal(a.step, b.step) and (a.block, a.degree, tuple(a.shape)) == (b.block, b.degree, tuple(b.shape)))


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
def test_tuner(pkg, dev, dtype):
    """five steps with TV on at a large rate of sigma (printed: how many sigmas reach 0, how many rows the repack drops): the losses,
    the moments and the repacked volume against Finetuner on the unpacked volume"""
    s = scene((9, 8, 7))
    cv = pkg.volume.pack(device_volume(pkg, dev, s, 2), dtype)
    rays = rays_on(dev, s)
    target = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 1.0, (NRAYS, 3)).astype(F)).to(dev)
    kw = dict(background=BG, dt=DT, t_stop=0.0)
    lrs = dict(lr_sigma=2.0, lr_coef=0.02, tv_sigma=2e-3, tv_coef=1e-3)
    keep = (cv.sigma.clone(), cv.coef.clone())
    ct, dt_ = pkg.volume.CompactFinetuner(cv, **lrs), pkg.volume.Finetuner(pkg.volume.unpack(cv), **lrs)
    assert ct.cvol.coef.dtype == torch.float32 and ct.cvol.coef.shape == (130, 27) and same(ct.point, dt_.index)
    for it in range(5):
        la, lb = ct.step(*rays, target, **kw), dt_.step(*rays, target, **kw)
        assert same(la, lb) and la.dim() == 0, it
    assert ct.steps == 5 and same(ct.m, dt_.m) and same(ct.v, dt_.v) and not ct.grad.acc_sigma.any() and not ct.grad.acc_coef.any()
    for out in ("fp32", "fp16"):
        got, want = ct.volume(out), pkg.volume.pack(dt_.volume(), out)
        assert same_compact(got, want) and got.coef.dtype == (torch.float16 if out == "fp16" else torch.float32)
    print(f"{dtype}: {int(cv.sigma.shape[0])} rows -> {int(got.sigma.shape[0])} after 5 steps; "
          f"{int(((ct.cvol.sigma == 0) & (keep[0] > 0)).sum())} sigmas reached 0")
    assert same(cv.sigma, keep[0]) and same(cv.coef, keep[1])                      # the tuner works on its own copies
    with pytest.raises(ValueError):
        ct.volume("fp8")


@pytest.fixture(scope="module")
def run(pkg, dev, tmp_path_factory):
    """the runner of tests/test_gpu_volume_compact.py::test_runner: the synthetic scene, one iteration, not trained"""
    tmp = str(tmp_path_factory.mktemp("compact_train"))
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    torch.manual_seed(0)
    return pkg.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/rs/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=1, batch_ray=256,
                          learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                          decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=1)


@pytest.mark.parametrize("prune", (0.0, 0.5))
def test_finetune_compact_schedule(pkg, dev, run, prune):
    """finetune_compact against pack(finetune(unpack)) with the same seed: six steps of 128 rays, the lattice doubled after step 3"""
    baked = run.model.bake_volume((-1.5,) * 3, (1.5,) * 3, 12, degree=1, block=4)
    if prune:
        prune = float(torch.quantile(baked.sigma[baked.sigma > 0], 0.3))           # a threshold that clears some of the density
    cv = pkg.volume.pack(baked)
    kw = dict(batch=128, seed=3, background=BG, upsample_at=(3,), prune=prune, lr_sigma=0.5, tv_sigma=1e-3, tv_coef=1e-3)
    got, losses = pkg.volume.finetune_compact(cv, run.train_rays, run.K_inv, 6, **kw)
    want, want_losses = pkg.volume.finetune(pkg.volume.unpack(cv), run.train_rays, run.K_inv, 6, **kw)
    assert isinstance(got, pkg.volume.CompactVolume) and got.shape == (23, 23, 23) and got.coef.dtype == torch.float32
    assert same(losses, want_losses) and losses.shape == (6,) and same_compact(got, pkg.volume.pack(want))
    assert got.sigma.shape[0] > 0 and bool((losses > 0).all())
    print(f"prune {prune:g}: {int(cv.sigma.shape[0])} rows of 12^3 -> {int(got.sigma.shape[0])} rows of 23^3")
    with pytest.raises(ValueError):
        pkg.volume.finetune_compact(cv, run.train_rays, run.K_inv, 6, upsample_at=(6,))


def test_memory(pkg, dev):
    """A CONDITION, not a measurement: on a (33, 33, 33) degree-2 lattice with positive sigma in a 3 x 3 x 3 clump (rule VA: 5^3 = 125
    rows), constructing the tuner, two steps of 130 rays and .volume() must raise the allocator's peak by less than ONE dense
    coefficient array, 35,937 x 27 x 4 B = 3,881,196 B.  What the layouts predict: per row 112 B parameters + 224 B accumulators +
    224 B moments + 4 B point = 564 B x 125 = 70.5 kB; transients of one lattice word each (the bool masks and indices of row_points,
    the repack's dense sigma, its slots and the active list's workspace) at 35,937 x 4 B = 144 kB apiece, a handful alive at once;
    the rays' buffers 130 x 60 B: under 0.6 MB in all.  A dense tuner's int64 coefficient accumulators alone are 7.76 MB."""
    shape, nc = (33, 33, 33), 9
    rng = np.random.default_rng(2)
    sigma = np.zeros(shape, F)
    sigma[15:18, 15:18, 15:18] = rng.uniform(1.0, 4.0, (3, 3, 3))
    lo, step = np.full(3, -1.0, F), np.full(3, 2.0 / 32, F)
    sg = torch.from_numpy(sigma).to(dev)
    index = pkg.volume.active(sg)
    n = int(index.shape[0])
    assert n == 125
    rows = torch.from_numpy(rng.normal(0.3, 0.3, (n, 3 * nc)).astype(F)).to(dev)
    cv = pkg.volume.CompactVolume(pkg.ops.volume_compact_slots(index, shape), sg.reshape(-1)[index.long()].contiguous(), rows,
                                  pkg.volume.blocks(sg, 8), lo, step, 8, 2, shape)
    o, d, tmin, tmax = (torch.from_numpy(np.ascontiguousarray(a[:130])).to(dev) for a in R.make_rays(NRAYS, 5, lo, step, shape))
    target = torch.from_numpy(rng.uniform(0.0, 1.0, (130, 3)).astype(F)).to(dev)
    del sg, index
    dense_coef_bytes = 35937 * 27 * 4
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    tuner = pkg.volume.CompactFinetuner(cv, tv_sigma=1e-3, tv_coef=1e-3)
    losses = [tuner.step(o, d, tmin, tmax, target, background=BG) for _ in range(2)]
    out = tuner.volume()
    torch.cuda.synchronize(dev)
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"allocator peak rose by {rise} B; one dense coefficient array is {dense_coef_bytes} B")
    assert rise < dense_coef_bytes == 3881196
    assert out.sigma.shape[0] == 125 and float(losses[0]) > 0 and not same(out.coef, cv.coef)          # it did train


def test_runner(pkg, dev, run, capsys):
    """--volume 12 --volume-compact fp16 --volume-finetune 2 with and without --volume-finetune-compact, as main.py passes them: the
    same files with the same arrays"""
    rs = run.results_path
    arrays = {}
    for flag in (False, True):
        capsys.readouterr()
        vol = run.bake_volume(12, compact="fp16", save=True, finetune=2, finetune_batch=128, finetune_compact=flag)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VOLUME]")]
        assert len(lines) == 2 and "compact fp16" in lines[0] and "2 steps of 128 train rays: batch loss" in lines[1]
        assert ("finetune compact 2 steps" in lines[1]) == flag and ("finetune 2 steps" in lines[1]) == (not flag)
        assert isinstance(vol, pkg.volume.CompactVolume) and vol.coef.dtype == torch.float16 and vol.shape == (12, 12, 12)
        names = sorted(os.path.basename(f) for f in glob.glob(rs + "*_volume12*.npz"))
        assert names == [f"{run.start_time}_{run.last_iter}_volume12_c16.npz", f"{run.start_time}_{run.last_iter}_volume12_ft2_c16.npz"]
        assert same_compact(pkg.volume.load(rs + names[1], dev), vol)
        for name in names:
            with np.load(rs + name) as z:
                arrays[flag, name] = {k: z[k] for k in z.files}
            os.remove(rs + name)
    for name in names:
        a, b = arrays[False, name], arrays[True, name]
        assert sorted(a) == sorted(b) == ["block", "coef_rows", "degree", "lo", "occ", "sigma_rows", "slot", "step"]
        assert all(same(a[k], b[k]) for k in a), name
    assert arrays[True, names[1]]["sigma_rows"].shape[0] > 0 and not same(arrays[True, names[0]]["coef_rows"], arrays[True, names[1]]["coef_rows"])
    for kw in (dict(finetune=2), dict(compact="fp16"), dict()):
        with pytest.raises(ValueError, match="finetune_compact"):
            run.bake_volume(12, save=False, finetune_compact=True, **kw)
    assert capsys.readouterr().out.count("[VOLUME]") == 0


def test_refusals(pkg, dev):
    L, f3 = pkg._abi.lib(), pkg._abi.f32_array
    s = scene((5, 4, 3))
    dv = device_volume(pkg, dev, s, 2)
    cv = pkg.volume.pack(dv)
    n, N = int(cv.sigma.shape[0]), 4
    lo, step, bg = f3(s["lo"].tolist()), f3(s["step"].tolist()), f3([0.0] * 3)
    o, d = torch.zeros(N, 3, device=dev), torch.ones(N, 3, device=dev)
    t0, t1 = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    g = torch.zeros(N, 3, device=dev)
    grad = pkg.volume.compact_grad_buffers(cv)
    point = pkg.volume.row_points(cv)
    m, v = torch.zeros(n, 28, device=dev), torch.zeros(n, 28, device=dev)
    P = lambda t: t.data_ptr()
    ERR = -1

    def bwd(**kw):
        a = dict(slot=P(cv.slot), srows=P(cv.sigma), crows=P(cv.coef), n=n, occ=P(cv.occ), nx=5, degree=2, block=2, N=N, dt=0.1,
                 acc_s=P(grad.acc_sigma), acc_c=P(grad.acc_coef), g=P(g))
        a.update(kw)
        return L.nerf_hip_volume_compact_render_backward(a["slot"], a["srows"], a["crows"], a["n"], a["occ"], a["nx"], 4, 3, a["degree"], a["block"],
                                                         lo, step, P(o), P(d), P(t0), P(t1), a["N"], a["dt"], 0.0, bg, a["g"], None, a["acc_s"],
                                                         a["acc_c"], None)

    def adam(**kw):
        a = dict(srows=P(cv.sigma), crows=P(cv.coef), n=n, degree=2, acc_s=P(grad.acc_sigma), acc_c=P(grad.acc_coef), m=P(m), step=1, beta1=0.9)
        a.update(kw)
        return L.nerf_hip_volume_compact_adam_step(a["srows"], a["crows"], a["n"], a["degree"], a["acc_s"], a["acc_c"], a["m"], P(v), 1.0,
                                                   a["step"], 0.0, 0.0, a["beta1"], 0.999, 1e-8, None)

    def tv(**kw):
        a = dict(slot=P(cv.slot), srows=P(cv.sigma), crows=P(cv.coef), point=P(point), n=n, nx=5, degree=2, w=1.0, eps=1e-9,
                 acc_s=P(grad.acc_sigma), acc_c=P(grad.acc_coef))
        a.update(kw)
        return L.nerf_hip_volume_compact_tv_backward(a["slot"], a["srows"], a["crows"], a["point"], a["n"], a["nx"], 4, 3, a["degree"], a["w"],
                                                     a["w"], a["eps"], a["acc_s"], a["acc_c"], None)

    assert bwd() == 0 and adam() == 0 and tv() == 0                                # (rates of 0: the rows keep their bits)
    torch.cuda.synchronize()
    assert same(cv.sigma, s["sigma"].reshape(-1)[s["index"]])
    common = [dict(n=61), dict(n=-1), dict(degree=3), dict(srows=None), dict(crows=None), dict(acc_s=None), dict(acc_c=None),
              dict(acc_s=P(grad.acc_sigma) + 4), dict(acc_c=P(grad.acc_coef) + 4)]
    for kw in common + [dict(slot=None), dict(nx=1), dict(block=0), dict(dt=0.0), dict(N=-1), dict(occ=None), dict(g=None)]:
        assert bwd(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in common[1:] + [dict(m=None), dict(step=0), dict(beta1=1.0)]:
        assert adam(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in common + [dict(slot=None), dict(nx=1), dict(point=None), dict(w=-1.0), dict(w=65537.0), dict(eps=0.0)]:
        assert tv(**kw) == ERR and L.nerf_hip_last_error(), kw
    # no rows: null row pointers are fine and nothing is launched
    empty = torch.full((5, 4, 3), -1, dtype=torch.int32, device=dev)
    no = dict(slot=P(empty), srows=None, crows=None, n=0, acc_s=None, acc_c=None)
    assert bwd(**no) == 0 and tv(point=None, **no) == 0 and adam(srows=None, crows=None, n=0, acc_s=None, acc_c=None, m=None) == 0
    assert bwd(N=0) == 0 and tv(w=0.0) == 0
    # the Python layer: host tensors, dense volumes, fp16 rows, accumulators of the wrong shape
    hostc = cv._replace(slot=cv.slot.cpu(), sigma=cv.sigma.cpu(), coef=cv.coef.cpu(), occ=cv.occ.cpu())
    Vm = pkg.volume
    for call in (lambda: Vm.compact_grad_buffers(hostc), lambda: Vm.compact_render_backward(hostc, grad, o, d, 0.0, 1.0, g),
                 lambda: Vm.compact_render_backward(cv, grad, o.cpu(), d, 0.0, 1.0, g), lambda: Vm.compact_tv_backward(hostc, grad, 1.0, 1.0),
                 lambda: Vm.CompactFinetuner(hostc), lambda: Vm.row_points(hostc), lambda: Vm.finetune_compact(hostc, None, None, 1)):
        with pytest.raises(RuntimeError, match="runs only on a ROCm device"):
            call()
    for call in (lambda: Vm.compact_grad_buffers(dv), lambda: Vm.compact_render_backward(dv, grad, o, d, 0.0, 1.0, g),
                 lambda: Vm.compact_tv_backward(dv, grad, 1.0, 1.0), lambda: Vm.CompactFinetuner(dv), lambda: Vm.row_points(dv),
                 lambda: Vm.finetune_compact(dv, None, None, 1)):
        with pytest.raises(TypeError, match="CompactVolume"):
            call()
    half = pkg.volume.pack(dv, "fp16")
    with pytest.raises(ValueError, match="fp32 rows"):
        Vm.compact_render_backward(half, grad, o, d, 0.0, 1.0, g)
    with pytest.raises(ValueError, match="fp32 rows"):
        Vm.compact_tv_backward(half, grad, 1.0, 1.0)
    with pytest.raises(ValueError):
        Vm.compact_render_backward(cv, Vm.CompactGrad(grad.acc_sigma[:-1].contiguous(), grad.acc_coef), o, d, 0.0, 1.0, g)
    with pytest.raises(ValueError):
        Vm.compact_render_backward(cv, Vm.CompactGrad(grad.acc_sigma.int(), grad.acc_coef), o, d, 0.0, 1.0, g)
    with pytest.raises(pkg._abi.NerfHipError):
        Vm.compact_render_backward(cv, grad, o, d, 0.0, 1.0, g, dt=0.0)
    with pytest.raises(pkg._abi.NerfHipError):
        Vm.compact_tv_backward(cv, grad, 1.0, 1.0, eps=0.0)
    with pytest.raises(ValueError):
        Vm.CompactFinetuner(cv, tv_sigma=-1.0)
    # the dense calls still refuse the compact form
    with pytest.raises(TypeError, match="unpack"):
        Vm.Finetuner(cv)
    with pytest.raises(TypeError, match="unpack"):
        Vm.render_backward(cv, grad, o, d, 0.0, 1.0, g)
