"""GPU: the SH radiance volume kernels (csrc/volume.hip) against the numpy restatement of their rules (tests/volume_reference.py):
bit for bit wherever no exp is involved, within the restatement's derived bound of the fp64 composite where one is; the bake against
the field's own queries; refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import volume_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))   # no multiple of a block edge; 60 .. 1836 points: one partial workgroup .. several
BLOCKS = (1, 2, 4, 8, 1 << 30)                   # the last: one block
NRAYS = 300                                      # 0, 1, 130 and 300 rays: none, one lane, partial waves
DT = F(0.04)                                     # the box's diagonal is 2.83: at most 71 samples a ray
BG = (0.25, 0.5, 1.0)
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view({4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def scene(shape):
    """the hand-made volume of a lattice, its rays and the restatement's march of them (computed once, never changed)"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        ref = R.march(sigma, coef, R.blocks(sigma, 2), 2, lo, step, o, d, tmin, tmax, DT, 0.0, BG)
        _cache[shape] = dict(sigma=sigma, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax, ref=ref)
    return _cache[shape]


def device_volume(pkg, dev, s, block, degree=2):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sigma = t(s["sigma"])
    nc = (degree + 1) ** 2
    return pkg.volume.Volume(sigma, t(s["coef"][..., :nc, :]), pkg.volume.blocks(sigma, block), s["lo"], s["step"],
                             min(block, pkg.volume.ONE_BLOCK), degree)


@pytest.mark.parametrize("shape", LATTICES)
def test_active_points_and_blocks(pkg, dev, shape):
    s = scene(shape)
    sigma = torch.from_numpy(s["sigma"]).to(dev)
    want = R.active(s["sigma"])
    got = pkg.volume.active(sigma)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want) and 0 < want.size < s["sigma"].size
    pts = pkg.ops.volume_points(got, shape, s["lo"].tolist(), s["step"].tolist())
    assert np.array_equal(bits(pts), bits(R.lattice_points(want, shape, s["lo"], s["step"])))
    # a chunk of the list, an empty list, and an index outside the lattice
    assert np.array_equal(bits(pkg.ops.volume_points(got[3:9], shape, s["lo"].tolist(), s["step"].tolist())), bits(pts[3:9]))
    assert pkg.ops.volume_points(got[:0], shape, s["lo"].tolist(), s["step"].tolist()).shape == (0, 3)
    bad = torch.tensor([-1, int(np.prod(shape))], dtype=torch.int32, device=dev)
    assert torch.isnan(pkg.ops.volume_points(bad, shape, s["lo"].tolist(), s["step"].tolist())).all()
    for B in BLOCKS:
        occ = pkg.volume.blocks(sigma, B)
        assert occ.dtype == torch.uint8 and np.array_equal(occ.cpu().numpy(), R.blocks(s["sigma"], B)), B
    # nothing positive (a NaN is not positive): no active point, no occupied block
    z = torch.zeros(shape, device=dev)
    z[1, 1, 1] = float("nan")
    z[0, 0, 0] = -1.0
    assert pkg.volume.active(z).numel() == 0 and not pkg.volume.blocks(z, 2).any()


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_sample(pkg, dev, shape, degree):
    s = scene(shape)
    vol = device_volume(pkg, dev, s, 2, degree)
    rng = np.random.default_rng(3)
    lo, step = s["lo"], s["step"]
    hi = (lo + (np.asarray(shape) - 1).astype(F) * step).astype(F)
    inside = (lo + rng.uniform(0, 1, (120, 3)) * (hi - lo)).astype(F)
    lattice = R.lattice_points(np.arange(int(np.prod(shape)))[::3], shape, lo, step)      # lattice points: the faces among them
    faces = inside[:24].copy()
    ax, low = np.arange(24) % 3, np.arange(24) % 2 == 0
    faces[np.arange(24), ax] = np.where(low, lo[ax], hi[ax])
    outside = (inside[:30] + np.asarray([2.5, 0, 0], F) * rng.choice([-1, 1], (30, 1))).astype(F)
    beyond = faces.copy()                                                                 # one ulp past a face
    beyond[np.arange(24), ax] = np.nextafter(beyond[np.arange(24), ax], np.where(low, -np.inf, np.inf).astype(F))
    weird = np.asarray([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3], F)
    x = np.concatenate([inside, lattice, faces, outside, beyond, weird]).astype(F)
    d = rng.normal(size=x.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[5] *= 1.7                                                                           # used as given, not renormalised
    d = d.astype(F)
    want_s, want_c = R.lookup(s["sigma"], s["coef"][..., :(degree + 1) ** 2, :], lo, step, x, d)
    got_s, got_c = pkg.volume.sample(vol, torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev))
    assert np.array_equal(bits(got_s), bits(want_s))
    assert np.array_equal(bits(got_c), bits(want_c))
    assert (want_s > 0).sum() > 20 and (want_c == 1).any() and (want_c == 0).any() and ((want_c > 0) & (want_c < 1)).any()
    e_s, e_c = pkg.volume.sample(vol, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev))
    assert e_s.shape == (0,) and e_c.shape == (0, 3)


def _check_bound(s, rgb, maps, info):
    worst = 0.0
    bgmax = max(abs(b) for b in BG)
    for r, (smp, used) in enumerate(info):
        if smp is None or not used:
            continue
        c64, m64 = R.composite64(smp, used, BG)
        b = R.bound(len(used))
        tmax = max(1.0, float(np.max(smp["tk"][used])))
        e = max(np.abs(rgb[r] - c64).max() / (b * (1 + bgmax)), abs(maps[r, 1] - m64[1]) / b, abs(maps[r, 0] - m64[0]) / (b * tmax))
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("shape", LATTICES)
def test_render(pkg, dev, shape):
    s = scene(shape)
    ref_rgb, ref_maps, ref_steps, info = s["ref"]
    t = lambda a: torch.from_numpy(a).to(dev)
    o, d, tmin, tmax = t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"])
    outs = {}
    for B in BLOCKS:
        vol = device_volume(pkg, dev, s, B)
        rgb, maps, steps = pkg.volume.render(vol, o, d, tmin, tmax, dt=DT, t_stop=0.0, background=BG)
        outs[B] = (rgb.cpu().numpy(), maps.cpu().numpy(), steps.cpu().numpy())
    rgb, maps, steps = outs[2]
    # bit for bit: the contributing counts and the miss pattern
    assert np.array_equal(steps[:, 0], ref_steps[:, 0])
    miss = np.asarray([smp is None for smp, _ in info])
    assert np.array_equal(steps[:, 1] == 0, miss)
    assert np.array_equal(bits(rgb[miss]), bits(np.broadcast_to(np.asarray(BG, F), (int(miss.sum()), 3))))
    assert not maps[miss].any() and not steps[miss].any() and miss.sum() >= NRAYS // 10
    # within the derived bound of the fp64 composite of the rule's own sample values
    worst = _check_bound(s, rgb, maps, info)
    print(f"{shape}: device march vs fp64 composite, worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    # the block edge changes only the samples looked at
    for B in BLOCKS:
        assert np.array_equal(bits(outs[B][0]), bits(rgb)) and np.array_equal(bits(outs[B][1]), bits(maps)), B
        assert np.array_equal(outs[B][2][:, 0], steps[:, 0]), B
    one = outs[BLOCKS[-1]][2][:, 1]
    assert (steps[:, 1] <= one).all() and steps[:, 1].sum() < one.sum() and (one <= 72).all()
    # 0, 1 and 130 rays: the same rays give the same bits whatever the launch holds
    vol = device_volume(pkg, dev, s, 2)
    for n in (0, 1, 130):
        r2, m2, s2 = pkg.volume.render(vol, o[:n], d[:n], tmin[:n], tmax[:n], dt=DT, t_stop=0.0, background=BG)
        assert r2.shape == (n, 3) and m2.shape == (n, 2) and s2.shape == (n, 2) and s2.dtype == torch.int32
        assert np.array_equal(bits(r2), bits(rgb[:n])) and np.array_equal(bits(m2), bits(maps[:n])) and np.array_equal(s2.cpu().numpy(), steps[:n])
    # lower degrees render from the leading coefficients: against the restatement's march of that slab
    for degree in (0, 1):
        nc = (degree + 1) ** 2
        want = R.march(s["sigma"], s["coef"][..., :nc, :], R.blocks(s["sigma"], 2), 2, s["lo"], s["step"], s["o"][:40], s["d"][:40], s["tmin"][:40],
                       s["tmax"][:40], DT, 0.0, BG)
        r2, m2, s2 = pkg.volume.render(device_volume(pkg, dev, s, 2, degree), o[:40], d[:40], tmin[:40], tmax[:40], dt=DT, t_stop=0.0, background=BG)
        assert np.array_equal(s2.cpu().numpy()[:, 0], want[2][:, 0])
        assert _check_bound(s, r2.cpu().numpy(), m2.cpu().numpy(), want[3]) <= 1.0


def test_analytic_slab(pkg, dev):
    sigma, coef, lo, step, o, d, tmin, tmax, dt, K, sigma0, c = R.slab_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sg = t(sigma)
    vol = pkg.volume.Volume(sg, t(coef), pkg.volume.blocks(sg, 2), lo, step, 2, 0)
    rgb, maps, steps = pkg.volume.render(vol, t(o), t(d), t(tmin), t(tmax), dt=dt, t_stop=0.0)
    R.check_slab(rgb.cpu().numpy(), maps.cpu().numpy(), steps.cpu().numpy(), K, sigma0, c, dt)


def test_t_stop_bound(pkg, dev):
    s = scene((9, 8, 7))
    vol = device_volume(pkg, dev, s, 2)
    t = lambda a: torch.from_numpy(a).to(dev)
    args = (t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"]))
    full = [a.cpu().numpy() for a in pkg.volume.render(vol, *args, dt=DT, t_stop=0.0, background=BG)]
    for t_stop in (1e-3, 0.3):
        rgb, maps, steps = (a.cpu().numpy() for a in pkg.volume.render(vol, *args, dt=DT, t_stop=t_stop, background=BG))
        assert np.abs(rgb.astype(np.float64) - full[0]).max() <= t_stop * (1 + max(abs(b) for b in BG))
        assert (steps[:, 0] <= full[2][:, 0]).all()
    assert (steps[:, 0] < full[2][:, 0]).any()
    # the default step is half the smallest lattice step
    assert pkg.volume.default_dt(vol) == float(F(0.5) * s["step"].min())
    a = pkg.volume.render(vol, *args, background=BG)
    b = pkg.volume.render(vol, *args, dt=pkg.volume.default_dt(vol), t_stop=1e-3, background=BG)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


BOX = ((-1.2, -1.0, -0.9), (1.1, 1.3, 1.0))
RES = (9, 8, 7)


@pytest.fixture(scope="module")
def baked(model):
    return model.bake_volume(*BOX, RES, degree=2, block=2)


def test_bake(pkg, dev, model, baked, tmp_path):
    grid = model.density_grid(*BOX, RES)
    assert np.array_equal(bits(baked.sigma), bits(grid)) and (grid > 0).any()
    assert baked.coef.shape == RES + (9, 3) and baked.degree == 2 and baked.block == 2
    assert np.array_equal(baked.occ.cpu().numpy(), R.blocks(grid.cpu().numpy(), 2))
    # the coefficients: rule VS fed with model.query's own colours along the 12 directions
    index = R.active(grid.cpu().numpy())
    dirs, _ = R.sh_tables()
    pts = torch.from_numpy(R.lattice_points(index, RES, baked.lo, baked.step)).to(dev)
    rgbs = [model.query(pts, torch.from_numpy(np.broadcast_to(dirs[k], (len(index), 3)).copy()).to(dev))[0].cpu().numpy() for k in range(12)]
    want = R.sh_project(rgbs, index, RES, 2)
    assert np.array_equal(bits(baked.coef), bits(want)) and index.size > 0
    inactive = np.ones(int(np.prod(RES)), bool)
    inactive[index] = False
    assert not baked.coef.cpu().numpy().reshape(-1, 27)[inactive].any()
    # lower degrees are the leading slabs; the chunking does not show
    for degree in (0, 1):
        v = model.bake_volume(*BOX, RES, degree=degree, block=2)
        assert np.array_equal(bits(v.coef), bits(baked.coef[..., :(degree + 1) ** 2, :].contiguous()))
    v64 = model.bake_volume(*BOX, RES, degree=2, block=2, points_per_call=64)
    assert np.array_equal(bits(v64.coef), bits(baked.coef)) and np.array_equal(bits(v64.sigma), bits(baked.sigma))
    # sigma_min: density_grid's bits at or above it, 0 below
    pos = grid[grid > 0]
    smin = float(pos.median()) if pos.numel() else 1.0
    vm = model.bake_volume(*BOX, RES, degree=0, sigma_min=smin)
    g = grid.cpu().numpy()
    assert np.array_equal(bits(vm.sigma), bits(np.where(g >= F(smin), g, F(0)))) and vm.block == 8
    # the file round-trips the bits
    path = str(tmp_path / "vol.npz")
    pkg.volume.save(path, baked)
    back = pkg.volume.load(path, dev)
    for a, b in zip(back[:3], baked[:3]):
        assert a.dtype == b.dtype and a.device == b.device and np.array_equal(bits(a), bits(b))
    assert np.array_equal(back.lo, baked.lo) and np.array_equal(back.step, baked.step) and (back.block, back.degree) == (2, 2)
    # and the baked volume renders: a view through it, finite, same bits from the loaded copy
    o = torch.tensor([[0.0, 0.1, -4.0]] * 64, device=dev)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.0, 1.0]], device=dev) + 0.2 * torch.rand(64, 3, device=dev), dim=1)
    r1 = pkg.volume.render(baked, o, d, 0.0, 10.0)
    r2 = pkg.volume.render(back, o, d, 0.0, 10.0)
    assert torch.isfinite(r1[0]).all() and all(np.array_equal(bits(a), bits(b)) for a, b in zip(r1, r2))


def test_render_views(pkg, dev):
    s = scene((9, 8, 7))
    vol = device_volume(pkg, dev, s, 2)
    P = np.zeros((2, 3, 5), np.float32)
    P[:, :, :3] = np.eye(3)
    P[:, :, 3] = [[0.5, 0.3, -3.0], [0.4, 0.2, -3.5]]
    pb = np.concatenate([P.reshape(2, 15), np.asarray([[1.0, 6.0], [2.0, 7.0]], np.float32)], axis=1)
    K_inv = torch.tensor([[0.0, 0.02, 0.0], [0.02, 0.0, 0.0], [-0.12, -0.1, 1.0]])  # (applied as the ray kernel applies it; only consistency matters)
    H, W = 12, 10
    rgb, maps, steps = pkg.volume.render_views(vol, pb, K_inv, H, W, dt=DT, t_stop=0.0, background=BG)
    assert rgb.shape == (2, H, W, 3) and maps.shape == (2, H, W, 2) and steps.shape == (2, H, W, 2)
    o, d = pkg.mesh.camera_rays(pb, K_inv, H, W, device=dev)
    near = torch.tensor([1.0, 2.0], device=dev).repeat_interleave(H * W)
    far = torch.tensor([6.0, 7.0], device=dev).repeat_interleave(H * W)
    want = pkg.volume.render(vol, o, d, near, far, dt=DT, t_stop=0.0, background=BG)
    assert np.array_equal(bits(rgb.reshape(-1, 3)), bits(want[0])) and np.array_equal(bits(maps.reshape(-1, 2)), bits(want[1]))
    assert np.array_equal(steps.reshape(-1, 2).cpu().numpy(), want[2].cpu().numpy())


def test_runner_bakes_saves_and_previews(pkg, dev, tmp_path, capsys):
    """NeRFRunner.bake_volume on one process: the file's name and bits, the preview frames, the [VOLUME] lines"""
    import glob

    scene = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    rs = str(tmp_path) + "/rs/"
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    vol = run.bake_volume(RES, lo=BOX[0], hi=BOX[1], degree=1, sigma_min=0.0, block=4, save=True, preview="test")
    out = capsys.readouterr().out
    assert out.count("[VOLUME]") == 2 and "9x8x7 degree 1" in out and "[PSNR]" in out and "[SSIM]" in out
    assert vol.coef.shape == RES + (4, 3) and vol.block == 4 and vol.degree == 1
    direct = run.model.bake_volume(*BOX, RES, degree=1, block=4)
    assert np.array_equal(bits(vol.sigma), bits(direct.sigma)) and np.array_equal(bits(vol.coef), bits(direct.coef))
    files = glob.glob(rs + "*_volume9x8x7.npz")
    assert len(files) == 1 and os.path.basename(files[0]) == f"{run.start_time}_{run.last_iter}_volume9x8x7.npz"
    back = pkg.volume.load(files[0], dev)
    assert np.array_equal(bits(back.coef), bits(vol.coef)) and np.array_equal(bits(back.sigma), bits(vol.sigma)) and back.degree == 1
    pngs = sorted(glob.glob(rs + run.start_time + "/*_volume.png"))
    assert [os.path.basename(p) for p in pngs] == ["0_volume.png", "1_volume.png"]
    assert all(open(p, "rb").read(8) == b"\x89PNG\r\n\x1a\n" for p in pngs)
    pv = run.last_volume_preview
    assert pv["views"] == 2 and np.isfinite(pv["psnr"]) and np.isfinite(pv["ssim"])
    # the preview's comparison frame is the model's own render of the view
    frame = pkg.volume.render_views(vol, run.disp_rays.poses[:1], run.K_inv, 16, 16)[0][0]
    m = pkg.metrics.image_metrics(frame, run.render_view(0, "disp")[0])
    p1 = pkg.metrics.image_metrics(pkg.volume.render_views(vol, run.disp_rays.poses[1:2], run.K_inv, 16, 16)[0][0], run.render_view(1, "disp")[0])
    assert abs(0.5 * (m["psnr"] + p1["psnr"]) - pv["psnr"]) < 1e-9
    # a cubic res names the file by its edge; no preview, no save: nothing more is written and one line is printed
    run.bake_volume(6, degree=0, save=False)
    assert capsys.readouterr().out.count("[VOLUME]") == 1 and len(glob.glob(rs + "*_volume*.npz")) == 1
    with pytest.raises(ValueError):
        run.bake_volume(6, preview="disp")


def test_points_refuses_a_host_index(pkg):
    with pytest.raises(ValueError):
        pkg.ops.volume_points(torch.zeros(3, dtype=torch.int32), (5, 4, 3), [0.0] * 3, [1.0] * 3)


def test_refusals(pkg, dev):
    L, abi = pkg._abi.lib(), pkg._abi
    s = scene((5, 4, 3))
    vol = device_volume(pkg, dev, s, 2)
    nx, ny, nz = 5, 4, 3
    f3 = abi.f32_array
    lo, step, bg = s["lo"].tolist(), s["step"].tolist(), [0.0, 0.0, 0.0]
    n = 4
    o = torch.zeros(n, 3, device=dev)
    d = torch.ones(n, 3, device=dev)
    t0, t1 = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    rgb, maps, steps = torch.empty(n, 3, device=dev), torch.empty(n, 2, device=dev), torch.empty(n, 2, dtype=torch.int32, device=dev)
    osig = torch.empty(n, device=dev)
    ws = torch.empty(abi.volume_ws_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    index = torch.zeros(n, dtype=torch.int32, device=dev)
    P = lambda t: t.data_ptr()

    def render(**kw):
        a = dict(sigma=P(vol.sigma), coef=P(vol.coef), occ=P(vol.occ), nx=nx, ny=ny, nz=nz, degree=2, block=2, lo=lo, step=step, o=P(o), d=P(d),
                 tmin=P(t0), tmax=P(t1), N=n, dt=0.1, t_stop=0.0, bg=bg, rgb=P(rgb), maps=P(maps), steps=P(steps))
        a.update(kw)
        return L.nerf_hip_volume_render(a["sigma"], a["coef"], a["occ"], a["nx"], a["ny"], a["nz"], a["degree"], a["block"], f3(a["lo"]),
                                        f3(a["step"]), a["o"], a["d"], a["tmin"], a["tmax"], a["N"], a["dt"], a["t_stop"], f3(a["bg"]),
                                        a["rgb"], a["maps"], a["steps"], None)

    def sample(**kw):
        a = dict(sigma=P(vol.sigma), coef=P(vol.coef), nx=nx, ny=ny, nz=nz, degree=2, lo=lo, step=step, x=P(o), d=P(d), M=n, os=P(osig), oc=P(rgb))
        a.update(kw)
        return L.nerf_hip_volume_sample(a["sigma"], a["coef"], a["nx"], a["ny"], a["nz"], a["degree"], f3(a["lo"]), f3(a["step"]), a["x"], a["d"],
                                        a["M"], a["os"], a["oc"], None)

    ERR = -1  # NERF_HIP_ERR_ARG
    assert render() == 0 and sample() == 0
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    bad_render = [dict(nx=1), dict(nz=1), dict(nx=2048, ny=1024, nz=1024), dict(degree=3), dict(degree=-1), dict(block=0),
                  dict(lo=[nan, 0, 0]), dict(lo=[0, inf, 0]), dict(step=[0.0, 1, 1]), dict(step=[1, -1.0, 1]), dict(step=[1, 1, inf]),
                  dict(step=[nan, 1, 1]), dict(dt=0.0), dict(dt=-1.0), dict(dt=inf), dict(dt=nan), dict(t_stop=1.0), dict(t_stop=-0.1),
                  dict(t_stop=nan), dict(bg=[nan, 0, 0]), dict(N=-1), dict(N=1 << 31), dict(sigma=None), dict(coef=None), dict(occ=None),
                  dict(o=None), dict(d=None), dict(tmin=None), dict(tmax=None), dict(rgb=None), dict(maps=None), dict(steps=None),
                  dict(sigma=P(vol.sigma) + 2), dict(o=P(o) + 1), dict(steps=P(steps) + 2)]
    for kw in bad_render:
        assert render(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in [dict(ny=1), dict(nx=2048, ny=1024, nz=1024), dict(degree=3), dict(lo=[0, 0, nan]), dict(step=[1, 0.0, 1]), dict(M=-1),
               dict(sigma=None), dict(coef=P(vol.coef) + 3), dict(x=None), dict(d=None), dict(os=None), dict(oc=None)]:
        assert sample(**kw) == ERR and L.nerf_hip_last_error(), kw
    # a count of 0 succeeds with null per-item pointers
    assert render(N=0, o=None, d=None, tmin=None, tmax=None, rgb=None, maps=None, steps=None) == 0
    assert sample(M=0, x=None, d=None, os=None, oc=None) == 0
    sg = P(vol.sigma)
    # active / points / accumulate / blocks
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, P(ws), ws.numel(), P(count), None) == 0
    assert L.nerf_hip_volume_active_count(sg, nx, 1, nz, P(ws), ws.numel(), P(count), None) == ERR
    assert L.nerf_hip_volume_active_count(sg, 2048, 1024, 1024, P(ws), ws.numel(), P(count), None) == ERR
    assert L.nerf_hip_volume_active_count(None, nx, ny, nz, P(ws), ws.numel(), P(count), None) == ERR
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, None, ws.numel(), P(count), None) == ERR
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, P(ws) + 4, ws.numel(), P(count), None) == ERR
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, P(ws), 8, P(count), None) == -2       # NERF_HIP_ERR_WORKSPACE
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, P(ws), ws.numel(), None, None) == ERR
    assert L.nerf_hip_volume_active_count(sg, nx, ny, nz, P(ws), ws.numel(), P(count) + 4, None) == ERR
    assert L.nerf_hip_volume_active_emit(sg, nx, ny, nz, P(ws), ws.numel(), P(index), -1, None) == ERR
    assert L.nerf_hip_volume_active_emit(sg, nx, ny, nz, P(ws), ws.numel(), None, n, None) == ERR
    assert L.nerf_hip_volume_active_emit(sg, nx, ny, nz, P(ws), ws.numel(), None, 0, None) == 0
    pts = torch.empty(n, 3, device=dev)
    assert L.nerf_hip_volume_points(P(index), n, nx, ny, nz, f3(lo), f3(step), P(pts), None) == 0
    assert L.nerf_hip_volume_points(P(index), n, nx, ny, 1, f3(lo), f3(step), P(pts), None) == ERR
    assert L.nerf_hip_volume_points(P(index), -1, nx, ny, nz, f3(lo), f3(step), P(pts), None) == ERR
    assert L.nerf_hip_volume_points(P(index), n, nx, ny, nz, f3([nan, 0, 0]), f3(step), P(pts), None) == ERR
    assert L.nerf_hip_volume_points(P(index), n, nx, ny, nz, f3(lo), f3([0.0, 1, 1]), P(pts), None) == ERR
    assert L.nerf_hip_volume_points(None, n, nx, ny, nz, f3(lo), f3(step), P(pts), None) == ERR
    assert L.nerf_hip_volume_points(P(index), n, nx, ny, nz, f3(lo), f3(step), None, None) == ERR
    assert L.nerf_hip_volume_points(None, 0, nx, ny, nz, f3(lo), f3(step), None, None) == 0
    coef = torch.zeros(nx, ny, nz, 9, 3, device=dev)
    assert L.nerf_hip_volume_sh_accumulate(P(coef), nx, ny, nz, 2, P(index), 1, P(rgb), 0, None) == 0
    for bad in [(P(coef), nx, ny, nz, 3, P(index), 1, P(rgb), 0), (P(coef), nx, ny, nz, 2, P(index), 1, P(rgb), 12),
                (P(coef), nx, ny, nz, 2, P(index), 1, P(rgb), -1), (P(coef), nx, ny, nz, 2, P(index), -1, P(rgb), 0),
                (None, nx, ny, nz, 2, P(index), 1, P(rgb), 0), (P(coef), nx, ny, nz, 2, None, 1, P(rgb), 0),
                (P(coef), nx, ny, nz, 2, P(index), 1, None, 0), (P(coef), 1, ny, nz, 2, P(index), 1, P(rgb), 0),
                (P(coef) + 2, nx, ny, nz, 2, P(index), 1, P(rgb), 0)]:
        assert L.nerf_hip_volume_sh_accumulate(*bad, None) == ERR, bad
    assert L.nerf_hip_volume_sh_accumulate(P(coef), nx, ny, nz, 2, None, 0, None, 0, None) == 0
    occ = torch.empty(2, 2, 1, dtype=torch.uint8, device=dev)
    assert L.nerf_hip_volume_blocks(sg, nx, ny, nz, 2, P(occ), None) == 0
    assert L.nerf_hip_volume_blocks(sg, nx, ny, nz, 0, P(occ), None) == ERR
    assert L.nerf_hip_volume_blocks(sg, nx, ny, 1, 2, P(occ), None) == ERR
    assert L.nerf_hip_volume_blocks(None, nx, ny, nz, 2, P(occ), None) == ERR
    assert L.nerf_hip_volume_blocks(sg, nx, ny, nz, 2, None, None) == ERR
    n_bytes = C.c_size_t(0)
    assert L.nerf_hip_volume_ws_bytes(1, ny, nz, C.byref(n_bytes)) == ERR and L.nerf_hip_volume_ws_bytes(nx, ny, nz, None) == ERR
    torch.cuda.synchronize()
    # the Python layer: CPU tensors raise, there is no CPU path
    cpu = pkg.volume.Volume(vol.sigma.cpu(), vol.coef.cpu(), vol.occ.cpu(), vol.lo, vol.step, 2, 2)
    with pytest.raises(RuntimeError):
        pkg.volume.render(cpu, o.cpu(), d.cpu(), 0.0, 1.0)
    with pytest.raises(RuntimeError):
        pkg.volume.sample(cpu, o.cpu(), d.cpu())
    with pytest.raises(RuntimeError):
        pkg.volume.blocks(vol.sigma.cpu(), 2)
    with pytest.raises(RuntimeError):
        pkg.volume.active(vol.sigma.cpu())
    with pytest.raises(RuntimeError):
        pkg.volume.render(vol, o.cpu(), d, 0.0, 1.0)
    with pytest.raises(RuntimeError):
        pkg.volume.load("nowhere.npz", "cpu")
    with pytest.raises(RuntimeError):
        pkg.NeRFModel(64, 128, 8).bake_volume(*BOX, RES)
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.volume.render(vol, o, d, 0.0, 1.0, dt=0.0)
