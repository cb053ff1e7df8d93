"""GPU: compact SH radiance volumes (csrc/volume_compact.hip; rule VC of include/nerf_hip.h) -- pack / unpack against the numpy
restatement (tests/volume_compact_reference.py) bit for bit, the lookup and the march through slots against the DENSE kernels on the
same device bit for bit (garbage at the dense volume's inactive points included: tests/test_volume_compact_cpu.py shows on the
restatement that it cannot reach the march), the compact bake against pack of the dense bake, the runner, refusals."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import volume_compact_reference as X
import volume_reference as R

sample_points = X.sample_points

pytestmark = pytest.mark.gpu

F = np.float32
LATTICES = ((5, 4, 3), (9, 8, 7), (17, 9, 12))   # 27 / 130 / 324 rows: one partial workgroup .. several
BLOCKS = (1, 2, 4, 8, 1 << 30)                   # the last: one block
NRAYS = 300
DT = F(0.04)
BG = (0.25, 0.5, 1.0)
DTYPES = ("fp32", "fp16")
_cache = {}


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.ascontiguousarray(a)


def bits(a):
    a = host(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    a, b = host(a), host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def scene(shape):
    """make_volume with garbage sigma at its inactive points (the coefficients are random everywhere) and the rays"""
    if shape not in _cache:
        sigma, coef, lo, step = R.make_volume(shape, seed=11)
        garbage, inactive = X.with_garbage(sigma, coef)
        o, d, tmin, tmax = R.make_rays(NRAYS, 5, lo, step, shape)
        _cache[shape] = dict(sigma=garbage, inactive=inactive, coef=coef, lo=lo, step=step, o=o, d=d, tmin=tmin, tmax=tmax)
    return _cache[shape]


def device_volume(pkg, dev, sigma, coef, lo, step, block=2):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sg = t(sigma)
    return pkg.volume.Volume(sg, t(coef), pkg.volume.blocks(sg, block), lo, step, min(block, pkg.volume.ONE_BLOCK), {1: 0, 4: 1, 9: 2}[coef.shape[3]])


def special_coefficients(coef, sigma):
    """coef with fp16's hard cases planted in the first active rows: ties, values that land on subnormal halves, +-65504, finite
    values past it, +-0, a NaN"""
    v = np.asarray([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 3e-6, -3e-6, 2.0 ** -14,
                    65504.0, -65504.0, 65519.0, 65520.0, 1e6, -1e6, 3e38, 0.0, -0.0, np.nan, 1e-30], F)
    out = coef.copy()
    nw = coef.shape[3] * 3
    flat = out.reshape(-1, nw)
    index = R.active(sigma)
    k = 0
    for r in index:
        for w in range(nw):
            flat[r, w] = v[k % len(v)]
            k += 1
        if k >= 3 * len(v):
            break
    return out


def same_but_nan(a, b):
    a, b = host(a), host(b)
    na, nb = np.isnan(a.astype(np.float32)), np.isnan(b.astype(np.float32))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_pack_and_unpack(pkg, dev, shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = special_coefficients(np.ascontiguousarray(s["coef"][..., :nc, :]), s["sigma"])
    vol = device_volume(pkg, dev, s["sigma"], coef, s["lo"], s["step"])
    for dtype in DTYPES:
        half = dtype == "fp16"
        want = X.pack(s["sigma"], coef, half)
        cv = pkg.volume.pack(vol, dtype)
        assert isinstance(cv, pkg.volume.CompactVolume) and cv.shape == shape and cv.degree == degree and cv.block == 2 and cv.occ is vol.occ
        assert cv.slot.dtype == torch.int32 and same(cv.slot, want.slot)
        assert same(cv.sigma, want.sigma) and cv.sigma.shape[0] == (27, 130, 324)[LATTICES.index(shape)]
        assert cv.coef.dtype == (torch.float16 if half else torch.float32) and same_but_nan(cv.coef, want.coef)
        assert np.isnan(want.coef.astype(F)).any()
        if half:
            assert np.isinf(want.coef.astype(F)).sum() >= 4 and not bits(cv.coef[:, 3 * nc:]).any()      # past 65504: +-inf; the pad: +0
        # unpack
        back = pkg.volume.unpack(cv)
        u_sigma, u_coef = X.unpack(want)
        assert isinstance(back, pkg.volume.Volume) and same(back.sigma, u_sigma) and same_but_nan(back.coef, u_coef)
        assert back.degree == degree and back.block == 2 and back.occ is vol.occ
        # pack(unpack(c)) == c on the device as well
        again = pkg.volume.pack(back, dtype)
        assert same(again.slot, cv.slot) and same(again.sigma, cv.sigma) and same_but_nan(again.coef, want.coef)
        # the identity index: every lattice point a row, in order
        _, rows = pkg.ops.volume_compact_pack(None, vol.coef, None, half)
        assert same_but_nan(rows, X.rows(coef.reshape(-1, 3 * nc), half))
        every = torch.arange(int(np.prod(shape)), dtype=torch.int32, device=dev)
        s_rows, rows2 = pkg.ops.volume_compact_pack(vol.sigma, vol.coef, every, half)
        assert same_but_nan(rows2, X.rows(coef.reshape(-1, 3 * nc), half)) and same_but_nan(s_rows, s["sigma"].reshape(-1))
        assert pkg.volume.nbytes(cv) == want.slot.nbytes + want.sigma.nbytes + want.coef.nbytes + vol.occ.numel()
    assert pkg.volume.nbytes(vol) == s["sigma"].nbytes + coef.nbytes + vol.occ.numel()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_sample(pkg, dev, shape, degree, dtype):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    cv = pkg.volume.pack(device_volume(pkg, dev, s["sigma"], coef, s["lo"], s["step"]), dtype)
    x, d = sample_points(shape, s["lo"], s["step"])
    xt, dt = torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev)
    got_s, got_c = pkg.volume.sample(cv, xt, dt)
    want_s, want_c = pkg.volume.sample(pkg.volume.unpack(cv), xt, dt)
    assert same(got_s, want_s) and same(got_c, want_c)
    # and the restatement of the rule
    ref_s, ref_c = X.lookup(X.pack(s["sigma"], coef, dtype == "fp16"), s["lo"], s["step"], x, d)
    assert same(got_s, ref_s) and same(got_c, ref_c)
    assert (ref_s > 0).sum() > 20 and (ref_c == 1).any() and (ref_c == 0).any() and ((ref_c > 0) & (ref_c < 1)).any()
    e_s, e_c = pkg.volume.sample(cv, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev))
    assert e_s.shape == (0,) and e_c.shape == (0, 3)


@pytest.mark.parametrize("degree", (0, 1, 2))
@pytest.mark.parametrize("shape", LATTICES)
def test_render(pkg, dev, shape, degree):
    s = scene(shape)
    nc = (degree + 1) ** 2
    coef = np.ascontiguousarray(s["coef"][..., :nc, :])
    t = lambda a: torch.from_numpy(a).to(dev)
    o, d, tmin, tmax = t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"])
    V = device_volume(pkg, dev, s["sigma"], coef, s["lo"], s["step"])
    assert torch.isnan(V.sigma).any() and (V.sigma < 0).any()                        # the garbage is there
    dense = {"fp32": V, "fp16": V._replace(coef=V.coef.half().float())}
    assert not same(dense["fp16"].coef, V.coef)
    for dtype in DTYPES:
        base = pkg.volume.pack(dense["fp32"], dtype)                                  # packed from the fp32 volume: pack rounds
        for B in BLOCKS:
            cv, dv = pkg.volume.with_block(base, B), pkg.volume.with_block(dense[dtype], B)
            assert same(cv.occ, dv.occ) and cv.block == dv.block
            for t_stop in (0.0, 0.3):
                got = pkg.volume.render(cv, o, d, tmin, tmax, dt=DT, t_stop=t_stop, background=BG)
                want = pkg.volume.render(dv, o, d, tmin, tmax, dt=DT, t_stop=t_stop, background=BG)
                assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]), (dtype, B, t_stop)
                if t_stop == 0.0:
                    full = want[2].cpu().numpy()
                if B == 2:
                    for n in (0, 1, 130):
                        g2 = pkg.volume.render(cv, o[:n], d[:n], tmin[:n], tmax[:n], dt=DT, t_stop=t_stop, background=BG)
                        assert g2[0].shape == (n, 3) and g2[1].shape == (n, 2) and g2[2].shape == (n, 2) and g2[2].dtype == torch.int32
                        assert same(g2[0], want[0][:n]) and same(g2[1], want[1][:n]) and same(g2[2], want[2][:n]), (dtype, n, t_stop)
        # the equalities are not over empty sets
        assert (full[:, 1] == 0).sum() >= NRAYS // 10 and full[:, 0].sum() >= 2000
    # fp16 is a different image, by little
    a = pkg.volume.render(pkg.volume.pack(V, "fp32"), o, d, tmin, tmax, dt=DT, t_stop=0.0, background=BG)[0]
    b = pkg.volume.render(pkg.volume.pack(V, "fp16"), o, d, tmin, tmax, dt=DT, t_stop=0.0, background=BG)[0]
    assert 0 < float((a - b).abs().max()) < 1e-3
    # the default step, through either form
    assert pkg.volume.default_dt(base) == pkg.volume.default_dt(V) == float(F(0.5) * s["step"].min())


def test_render_views(pkg, dev):
    s = scene((9, 8, 7))
    V = device_volume(pkg, dev, s["sigma"], s["coef"], s["lo"], s["step"])
    P = np.zeros((2, 3, 5), np.float32)
    P[:, :, :3] = np.eye(3)
    P[:, :, 3] = [[0.5, 0.3, -3.0], [0.4, 0.2, -3.5]]
    pb = np.concatenate([P.reshape(2, 15), np.asarray([[1.0, 6.0], [2.0, 7.0]], np.float32)], axis=1)
    K_inv = torch.tensor([[0.0, 0.02, 0.0], [0.02, 0.0, 0.0], [-0.12, -0.1, 1.0]])
    want = pkg.volume.render_views(V, pb, K_inv, 12, 10, dt=DT, t_stop=0.0, background=BG)
    got = pkg.volume.render_views(pkg.volume.pack(V), pb, K_inv, 12, 10, dt=DT, t_stop=0.0, background=BG)
    assert got[0].shape == (2, 12, 10, 3) and all(same(a, b) for a, b in zip(got, want)) and int(want[2][..., 0].sum()) > 0


def test_edge_volumes(pkg, dev):
    shape = (9, 8, 7)
    s = scene(shape)
    t = lambda a: torch.from_numpy(a).to(dev)
    o, d, tmin, tmax = t(s["o"]), t(s["d"]), t(s["tmin"]), t(s["tmax"])
    x, dd = (t(a) for a in sample_points(shape, s["lo"], s["step"]))
    render = lambda v: pkg.volume.render(v, o, d, tmin, tmax, dt=DT, t_stop=0.0, background=BG)
    # nothing positive: no row at all
    nothing = np.zeros(shape, F)
    nothing[1, 1, 1], nothing[0, 0, 0], nothing[2, 3, 4] = np.nan, -1.0, -0.0
    V0 = device_volume(pkg, dev, nothing, s["coef"], s["lo"], s["step"])
    for dtype in DTYPES:
        c0 = pkg.volume.pack(V0, dtype)
        assert c0.sigma.shape == (0,) and c0.coef.shape == (0, 28 if dtype == "fp16" else 27) and (c0.slot == -1).all()
        rgb, maps, steps = render(c0)
        want = render(V0)
        assert same(rgb, want[0]) and same(maps, want[1]) and same(steps, want[2])
        assert same(rgb, np.broadcast_to(np.asarray(BG, F), (NRAYS, 3))) and not maps.any() and not steps[:, 0].any() and steps[:, 1].any()
        sg, col = pkg.volume.sample(c0, x, dd)
        assert not sg.any() and not col.any()
        u0 = pkg.volume.unpack(c0)
        assert not u0.sigma.any() and not u0.coef.any()
    # every point active: the slots count the lattice
    sigma, coef, lo, step = R.make_volume(shape, seed=11, empty_half=False)
    V1 = device_volume(pkg, dev, sigma, coef, lo, step)
    for dtype in DTYPES:
        c1 = pkg.volume.pack(V1, dtype)
        assert same(c1.slot, np.arange(sigma.size, dtype=np.int32).reshape(shape)) and same(c1.sigma, sigma.reshape(-1))
        want = render(V1 if dtype == "fp32" else V1._replace(coef=V1.coef.half().float()))
        assert all(same(a, b) for a, b in zip(render(c1), want)) and int(want[2][:, 0].sum()) > 2000
    # two slots outside [0, n): n itself and -2 -- those corners are inactive, whatever lies next to the rows
    V = device_volume(pkg, dev, s["sigma"], s["coef"], s["lo"], s["step"])
    for dtype in DTYPES:
        cv = pkg.volume.pack(V, dtype)
        n = int(cv.sigma.shape[0])
        pts = np.argsort(np.nan_to_num(s["sigma"].reshape(-1), nan=-1.0))[[-1, -5]]          # two points of the blob
        assert (s["sigma"].reshape(-1)[pts] > 0).all()
        slot = cv.slot.clone()
        slot.view(-1)[int(pts[0])] = n
        slot.view(-1)[int(pts[1])] = -2
        bad = cv._replace(slot=slot)
        dropped = pkg.volume.unpack(cv)
        dropped.sigma.view(-1)[torch.from_numpy(pts).to(dev)] = 0.0
        dropped.coef.view(-1, 27)[torch.from_numpy(pts).to(dev)] = 0.0
        ub = pkg.volume.unpack(bad)
        assert same(ub.sigma, dropped.sigma) and same(ub.coef, dropped.coef)
        got, want, whole = render(bad), render(dropped), render(cv)
        assert all(same(a, b) for a, b in zip(got, want)) and not same(got[0], whole[0])
        gs, ws, os_ = pkg.volume.sample(bad, x, dd), pkg.volume.sample(dropped, x, dd), pkg.volume.sample(cv, x, dd)
        assert same(gs[0], ws[0]) and same(gs[1], ws[1]) and not same(gs[0], os_[0])


@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(oracle.make_weights(5, False))
    return m.to(dev)


BOX = ((-1.2, -1.0, -0.9), (1.1, 1.3, 1.0))
RES = (9, 8, 7)
BIG = (24, 20, 22)


@pytest.fixture(scope="module")
def baked(model):
    return model.bake_volume(*BOX, RES, degree=2, block=2)


def same_compact(a, b):
    return (same(a.slot, b.slot) and same(a.sigma, b.sigma) and same(a.coef, b.coef) and same(a.occ, b.occ) and np.array_equal(a.lo, b.lo)
            and np.array_equal(a.step, b.step) and (a.block, a.degree, tuple(a.shape)) == (b.block, b.degree, tuple(b.shape)))


def test_bake(pkg, dev, model, baked, tmp_path):
    for dtype in DTYPES:
        want = pkg.volume.pack(baked, dtype)
        got = model.bake_volume(*BOX, RES, degree=2, block=2, compact=dtype)
        assert isinstance(got, pkg.volume.CompactVolume) and same_compact(got, want) and got.sigma.shape[0] > 0
        assert same_compact(model.bake_volume(*BOX, RES, degree=2, block=2, compact=dtype, points_per_call=64), want)
        low = model.bake_volume(*BOX, RES, degree=1, block=2, compact=dtype)
        assert same_compact(low, pkg.volume.pack(model.bake_volume(*BOX, RES, degree=1, block=2), dtype))
        # the file round-trips the bits, and says which form it holds
        path = str(tmp_path / f"c_{dtype}.npz")
        pkg.volume.save(path, got)
        back = pkg.volume.load(path, dev)
        assert isinstance(back, pkg.volume.CompactVolume) and same_compact(back, got) and back.coef.device == got.coef.device
    path = str(tmp_path / "dense.npz")
    pkg.volume.save(path, baked)
    assert sorted(np.load(path).files) == ["block", "coef", "degree", "lo", "occ", "sigma", "step"]      # today's file
    back = pkg.volume.load(path, dev)
    assert isinstance(back, pkg.volume.Volume) and same(back.sigma, baked.sigma) and same(back.coef, baked.coef)
    # a threshold: an empty lattice region, and nothing at all
    grid = model.density_grid(*BOX, RES)
    smin = float(grid[grid > 0].median())
    assert same_compact(model.bake_volume(*BOX, RES, sigma_min=smin, compact="fp16"), pkg.volume.pack(model.bake_volume(*BOX, RES, sigma_min=smin), "fp16"))
    none = model.bake_volume(*BOX, RES, sigma_min=float(grid.max()) * 2 + 1, compact="fp16")
    assert none.sigma.shape == (0,) and none.coef.shape == (0, 28) and (none.slot == -1).all()
    with pytest.raises(ValueError):
        model.bake_volume(*BOX, RES, compact="fp8")


def test_bake_peak_memory(pkg, dev, model):
    """the compact bake never holds the dense coefficient array: its allocator peak stays below the dense bake's at the same lattice.
    Per point the dense bake holds 4 + 108 bytes; the compact fp16 bake holds 4 (sigma) + 4 (slot) per point and 108 + 56 + 4 per ROW
    while it converts, so it wins below about 0.6 rows per point: the threshold keeps the densest 2 % of the field, whose 3 x 3 x 3
    neighbourhoods are the rows (printed)."""
    grid = model.density_grid(*BOX, BIG)
    smin = float(torch.quantile(grid[grid > 0], 0.98))
    model.bake_volume(*BOX, BIG, sigma_min=smin)                                      # the query workspace exists from here on
    del grid

    def peak(**kw):
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        v = model.bake_volume(*BOX, BIG, sigma_min=smin, **kw)
        torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev) - before, v

    p_dense, vd = peak()
    npts = int(np.prod(BIG))
    for dtype in DTYPES:
        p_c, vc = peak(compact=dtype)
        n = int(vc.sigma.shape[0])
        print(f"{BIG} {dtype}: {n} / {npts} rows; allocator peak dense {p_dense} B, compact {p_c} B; stored dense {pkg.volume.nbytes(vd)} B, "
              f"compact {pkg.volume.nbytes(vc)} B")
        assert 0 < n < npts and p_c < p_dense and pkg.volume.nbytes(vc) < pkg.volume.nbytes(vd)


LEGACY_LINE = r"^\[VOLUME\] -?\d+ 24x24x24 degree 2: \d+ / 13824 lattice points hold colour, \d+ / 27 blocks of 8 occupied, [\d.]+ MiB, [\d.]+ s$"


def test_runner(pkg, dev, tmp_path, capsys):
    """--volume 24 --volume-compact fp16 --volume-preview through NeRFRunner.bake_volume, as main.py passes them"""
    scene_ = pkg.data.synthetic_scene(n_pic=2, H=16, W=16)
    rs = str(tmp_path) + "/rs/"
    torch.manual_seed(0)
    run = pkg.NeRFRunner(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256,
                         learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
                         decay_end=10000, sched="EXP", continue_=False, datasets={"train": scene_, "val": scene_, "test": scene_}, log_every=1)
    capsys.readouterr()
    vol = run.bake_volume(24, compact="fp16", preview="test", save=True)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("[VOLUME]")]
    assert len(lines) == 2 and "[PSNR]" in lines[1] and "[SSIM]" in lines[1]
    both = [re.search(r"compact fp16 (\d+) bytes \(dense (\d+) bytes\)", ln) for ln in lines]
    assert both[0] and not both[1]
    assert isinstance(vol, pkg.volume.CompactVolume) and vol.coef.dtype == torch.float16
    assert int(both[0].group(1)) == pkg.volume.nbytes(vol) and int(both[0].group(2)) == 13824 * 112 + 27
    files = glob.glob(rs + "*_volume24*.npz")
    assert [os.path.basename(f) for f in files] == [f"{run.start_time}_{run.last_iter}_volume24_c16.npz"]
    assert same_compact(pkg.volume.load(files[0], dev), vol)
    direct = run.model.bake_volume((-1.5,) * 3, (1.5,) * 3, 24)
    assert same_compact(vol, pkg.volume.pack(direct, "fp16"))
    pngs = sorted(glob.glob(rs + run.start_time + "/*_volume.png"))
    assert [os.path.basename(p) for p in pngs] == ["0_volume.png", "1_volume.png"]
    # the preview frames come from the compact form
    frame = pkg.volume.render_views(vol, run.disp_rays.poses[:1], run.K_inv, 16, 16)[0][0]
    m0 = pkg.metrics.image_metrics(frame, run.render_view(0, "disp")[0])
    m1 = pkg.metrics.image_metrics(pkg.volume.render_views(vol, run.disp_rays.poses[1:2], run.K_inv, 16, 16)[0][0], run.render_view(1, "disp")[0])
    assert abs(0.5 * (m0["psnr"] + m1["psnr"]) - run.last_volume_preview["psnr"]) < 1e-9
    # without the argument: today's lines, today's file, the dense form
    for f in files:
        os.remove(f)
    capsys.readouterr()
    dense = run.bake_volume(24, preview="test", save=True)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VOLUME]")]
    assert len(lines) == 2 and re.match(LEGACY_LINE, lines[0]) and "compact" not in lines[0] + lines[1]
    assert isinstance(dense, pkg.volume.Volume) and same(dense.coef, direct.coef)
    files = glob.glob(rs + "*_volume24*.npz")
    assert [os.path.basename(f) for f in files] == [f"{run.start_time}_{run.last_iter}_volume24.npz"]
    assert isinstance(pkg.volume.load(files[0], dev), pkg.volume.Volume)
    # with fine-tuning: trained dense, packed before it is written
    ft = run.bake_volume(12, compact="fp32", save=True, finetune=2, finetune_batch=128)
    assert isinstance(ft, pkg.volume.CompactVolume) and ft.coef.dtype == torch.float32 and ft.shape == (12, 12, 12)
    names = sorted(os.path.basename(f) for f in glob.glob(rs + "*_volume12*.npz"))
    assert names == [f"{run.start_time}_{run.last_iter}_volume12_c32.npz", f"{run.start_time}_{run.last_iter}_volume12_ft2_c32.npz"]
    assert same_compact(pkg.volume.load(rs + names[1], dev), ft)
    with pytest.raises(ValueError):
        run.bake_volume(6, compact="fp8")


def test_refusals(pkg, dev):
    L, f3 = pkg._abi.lib(), pkg._abi.f32_array
    s = scene((5, 4, 3))
    V = device_volume(pkg, dev, s["sigma"], s["coef"], s["lo"], s["step"])
    cv = pkg.volume.pack(V, "fp16")
    n, N = int(cv.sigma.shape[0]), 4
    lo, step, bg = f3(s["lo"].tolist()), f3(s["step"].tolist()), f3([0.0] * 3)
    o, d = torch.zeros(N, 3, device=dev), torch.ones(N, 3, device=dev)
    t0, t1 = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    rgb, maps, steps = torch.empty(N, 3, device=dev), torch.empty(N, 2, device=dev), torch.empty(N, 2, dtype=torch.int32, device=dev)
    osig = torch.empty(N, device=dev)
    P = lambda t: t.data_ptr()

    def render(**kw):
        a = dict(slot=P(cv.slot), srows=P(cv.sigma), crows=P(cv.coef), n=n, half=1, occ=P(cv.occ), nx=5, degree=2, block=2, N=N, dt=0.1)
        a.update(kw)
        return L.nerf_hip_volume_compact_render(a["slot"], a["srows"], a["crows"], a["n"], a["half"], a["occ"], a["nx"], 4, 3, a["degree"],
                                                a["block"], lo, step, P(o), P(d), P(t0), P(t1), a["N"], a["dt"], 0.0, bg, P(rgb), P(maps),
                                                P(steps), None)

    def sample(**kw):
        a = dict(slot=P(cv.slot), srows=P(cv.sigma), crows=P(cv.coef), n=n, half=1, nx=5, degree=2, M=N)
        a.update(kw)
        return L.nerf_hip_volume_compact_sample(a["slot"], a["srows"], a["crows"], a["n"], a["half"], a["nx"], 4, 3, a["degree"], lo, step, P(o),
                                                P(d), a["M"], P(osig), P(rgb), None)

    ERR = -1
    assert render() == 0 and sample() == 0
    torch.cuda.synchronize()
    common = [dict(half=2), dict(half=-1), dict(n=61), dict(n=-1), dict(crows=P(cv.coef) + 4), dict(crows=P(cv.coef) + 2, half=0), dict(nx=1),
              dict(degree=3), dict(slot=None), dict(srows=None), dict(crows=None), dict(slot=P(cv.slot) + 2)]
    for kw in common + [dict(block=0), dict(dt=0.0), dict(N=-1), dict(occ=None)]:
        assert render(**kw) == ERR and L.nerf_hip_last_error(), kw
    for kw in common + [dict(M=-1)]:
        assert sample(**kw) == ERR and L.nerf_hip_last_error(), kw
    # no rows: null row pointers are fine
    empty = torch.full((5, 4, 3), -1, dtype=torch.int32, device=dev)
    assert render(slot=P(empty), srows=None, crows=None, n=0) == 0 and sample(slot=P(empty), srows=None, crows=None, n=0) == 0
    assert render(N=0) == 0 and sample(M=0) == 0
    torch.cuda.synchronize()
    assert same(rgb, np.zeros((N, 3), F)) and not osig.any()
    # the Python layer: a host tensor raises, the training calls point to unpack
    host = cv._replace(slot=cv.slot.cpu(), sigma=cv.sigma.cpu(), coef=cv.coef.cpu(), occ=cv.occ.cpu())
    for call in (lambda: pkg.volume.render(host, o.cpu(), d.cpu(), 0.0, 1.0), lambda: pkg.volume.sample(host, o.cpu(), d.cpu()),
                 lambda: pkg.volume.render(cv, o.cpu(), d, 0.0, 1.0), lambda: pkg.volume.unpack(host), lambda: pkg.volume.pack(V._replace(sigma=V.sigma.cpu()))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        pkg.ops.volume_compact_slots(torch.zeros(3, dtype=torch.int32), (5, 4, 3))
    with pytest.raises(ValueError):
        pkg.volume.render(cv._replace(coef=cv.coef[:, :27].contiguous()), o, d, 0.0, 1.0)          # not the rule's padded width
    with pytest.raises(TypeError, match="unpack"):
        pkg.volume.Finetuner(cv)
    with pytest.raises(TypeError, match="unpack"):
        pkg.volume.render_train(cv, o, d, 0.0, 1.0)
    with pytest.raises(pkg._abi.NerfHipError):
        pkg.volume.render(cv, o, d, 0.0, 1.0, dt=0.0)
    # and the way back works
    tuner = pkg.volume.Finetuner(pkg.volume.unpack(cv))
    assert tuner.index.shape[0] == n
