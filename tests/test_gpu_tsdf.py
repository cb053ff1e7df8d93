"""GPU: TSDF fusion on the device (nerf_hip_tsdf_integrate; mesh.tsdf_volume / tsdf_integrate / tsdf_grid; NeRFModel.fuse_depth /
extract_mesh_tsdf; NeRFRunner.extract_mesh(tsdf_from=)) against the numpy restatement of rule T in tests/tsdf_reference.py.  The volumes
are compared as bits."""
import ctypes
import glob

import numpy as np
import pytest
import torch

import tsdf_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the scenes are read-only)


def _same(got, want):
    """a device fp32 tensor and a numpy fp32 array, bit for bit"""
    return got.dtype == torch.float32 and torch.equal(got.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want, F32)).view(torch.int32))


def _fuse(pkg, dev, s, T=None, Wt=None, views=slice(None), opacity=True, **kw):
    if T is None:
        T, Wt = pkg.mesh.tsdf_volume(s["shape"], dev)
    return pkg.mesh.tsdf_integrate(T, Wt, s["lo"], s["step"], _t(s["depth"][views], dev), np.ascontiguousarray(s["poses"][views]), s["K"],
                                   opacity=_t(s["opacity"][views], dev) if opacity else None, trunc=s["trunc"], **kw)


# ---- (1) bit identity on a small lattice with every kind of bad depth ----

@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("with_opacity", [True, False])
def test_random_case_bit_identical(pkg, dev, carve, with_opacity):
    s = R.random_case()  # 5 x 6 x 7 lattice, 3 cameras, 8 x 12 images
    assert s["H"] != s["W"] and np.isnan(s["depth"]).any() and np.isinf(s["depth"]).any() and (s["depth"] == 0).any() and (s["depth"] < 0).any()
    z = np.zeros(s["shape"], F32)
    op = s["opacity"] if with_opacity else None
    want = R.integrate(z, z, s["lo"], s["step"], s["depth"], op, s["cams"], s["trunc"], 0.5, carve)
    T, Wt = _fuse(pkg, dev, s, opacity=with_opacity, carve=carve)
    assert tuple(T.shape) == s["shape"] and _same(T, want[0]) and _same(Wt, want[1])
    assert (want[1] > 0).any() and (want[1] >= 2).any()
    # a second call continues from the state the first left (the views in reverse order, another min_opacity)
    rev = slice(None, None, -1)
    want2 = R.integrate(want[0], want[1], s["lo"], s["step"], s["depth"][rev], None if op is None else op[rev], s["cams"][rev], s["trunc"], 0.3, carve)
    T2, Wt2 = _fuse(pkg, dev, s, T, Wt, views=rev, opacity=with_opacity, carve=carve, min_opacity=0.3)
    assert T2 is T and Wt2 is Wt and _same(T, want2[0]) and _same(Wt, want2[1]) and not np.array_equal(want2[1], want[1])


# ---- (2) the grouping of the views into launches and calls changes nothing ----

def test_grouping_into_launches_and_calls(pkg, dev):
    n = 2 * pkg._abi.TSDF_VIEWS_PER_LAUNCH + 1
    s = R.random_case(n=n, H=4, W=6, seed=1)
    z = np.zeros(s["shape"], F32)
    want = R.integrate(z, z, s["lo"], s["step"], s["depth"], s["opacity"], s["cams"], s["trunc"], 0.5, True)
    T, Wt = _fuse(pkg, dev, s)
    assert _same(T, want[0]) and _same(Wt, want[1]) and want[1].max() > pkg._abi.TSDF_VIEWS_PER_LAUNCH
    T1, Wt1 = pkg.mesh.tsdf_volume(s["shape"], dev)
    for c in range(n):
        _fuse(pkg, dev, s, T1, Wt1, views=slice(c, c + 1))
    assert _same(T1, want[0]) and _same(Wt1, want[1])


# ---- (3) cameras inside the lattice, on a lattice point, and with a frame that covers a part of it ----

def test_edge_cameras(pkg, dev):
    s = dict(R.random_case())
    P = R.lattice(s["lo"], s["step"], s["shape"])
    H, W = s["H"], s["W"]
    at_point = P[2, 3, 3]
    poses = np.stack([R.look_at((0.1, 0.05, -0.2), (1.0, 0.2, -0.1)),       # inside the lattice: voxels behind it
                      R.look_at(at_point.astype(np.float64), (1.0, 1.0, 1.0)),  # exactly on a lattice point
                      R.look_at((0.0, -3.0, 0.2), (0.3, 0.0, 0.2))])        # outside, with a narrow frame
    poses[1, [3, 8, 13]] = at_point  # (the position bit for bit)
    Ks = [R.k_inv(H, W, 0.3), R.k_inv(H, W, 0.3), R.k_inv(H, W, 0.06)]
    depth = np.full((1, H, W), 1.25, F32)
    z = np.zeros(s["shape"], F32)
    total_t, total_w = z, z
    T, Wt = pkg.mesh.tsdf_volume(s["shape"], dev)
    for c in range(3):
        cams = [R.camera_q(poses[c], Ks[c])]
        one = R.integrate(z, z, s["lo"], s["step"], depth, None, cams, s["trunc"], 0.5, True)
        seen = one[1] > 0
        print(f"camera {c}: {int(seen.sum())} of {seen.size} voxels observed")
        assert 0 < seen.sum() < seen.size
        if c == 1:
            assert one[1][2, 3, 3] == 0 and one[0][2, 3, 3] == 0  # m_2 > 0 is false at the camera itself
        t1, w1 = pkg.mesh.tsdf_volume(s["shape"], dev)
        pkg.mesh.tsdf_integrate(t1, w1, s["lo"], s["step"], _t(depth, dev), poses[c:c + 1], Ks[c], trunc=s["trunc"])
        assert _same(t1, one[0]) and _same(w1, one[1])
        total_t, total_w = R.integrate(total_t, total_w, s["lo"], s["step"], depth, None, cams, s["trunc"], 0.5, True)
        pkg.mesh.tsdf_integrate(T, Wt, s["lo"], s["step"], _t(depth, dev), poses[c:c + 1], Ks[c], trunc=s["trunc"])
    assert _same(T, total_t) and _same(Wt, total_w)
    none = total_w == 0
    assert none.any() and not T.cpu().numpy()[none].any() and not Wt.cpu().numpy()[none].any()  # what no view observes stays (0, 0)
    behind = ((P.astype(np.float64) - poses[0, [3, 8, 13]]) @ poses[0, [2, 7, 12]].astype(np.float64)) < 0
    w0 = R.integrate(z, z, s["lo"], s["step"], depth, None, [R.camera_q(poses[0], Ks[0])], s["trunc"], 0.5, True)[1]
    assert behind.sum() > 10 and not w0[behind].any()


# ---- (4) the sphere: fused volume, zero crossings, a closed mesh of one component ----

def test_sphere_scene_to_mesh(pkg, dev):
    s = R.sphere_scene()
    want = R.sphere_fused(True)
    T, Wt = _fuse(pkg, dev, s)
    assert _same(T, want[0]) and _same(Wt, want[1])
    G = pkg.mesh.tsdf_grid(T, Wt)
    assert _same(G, R.grid(*want))
    verts, faces, nrm = pkg.mesh.marching_cubes(G, 0.0, s["lo"], s["step"])
    v = verts.cpu().numpy().astype(np.float64)
    off = np.abs(np.linalg.norm(v, axis=1) - R.SPHERE_R) / float(s["step"].max())
    topo = pkg.mesh.topology(faces, len(verts))
    comps = pkg.mesh.components(faces, len(verts))
    print(f"sphere: V {len(verts)} F {len(faces)}, the farthest vertex {off.max():.3f} steps from the sphere; {topo.summary()}; {len(comps.n_faces)} component(s)")
    assert len(verts) >= 1 and off.max() <= 1.0
    assert topo.closed and len(comps.n_faces) == 1
    assert (np.einsum("ij,ij->i", nrm.cpu().numpy(), v / np.linalg.norm(v, axis=1, keepdims=True)) > 0.8).all()  # outward
    # the opposite defaults: a second sheet one truncation distance behind the surface
    T2, Wt2 = _fuse(pkg, dev, s, carve=False)
    w2 = R.sphere_fused(False)
    assert _same(T2, w2[0]) and _same(Wt2, w2[1])
    v2 = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T2, Wt2, unseen="empty"), 0.0, s["lo"], s["step"])[0].cpu().numpy().astype(np.float64)
    assert (np.abs(np.linalg.norm(v2, axis=1) - R.SPHERE_R) > 2.0 * float(s["step"].max())).any()


# ---- (5) the model's plumbing on the smallest fixture ----

@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    g = load_golden("small_16_32")
    m = pkg.NeRFModel(int(g["Nc"]), int(g["Nf"]), 8)
    m.load_state_dict(oracle.make_weights(int(g["seed"]), bool(g["sharp"])))
    return m.to(dev)


LO, HI, RES, VH, VW = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 6, 8, 10


def _views(dev):
    poses = np.stack([R.look_at((2.6, 0.3, 0.4), (0, 0, 0), near=1.0, far=4.5), R.look_at((-0.5, -2.4, 1.0), (0, 0, 0), near=1.2, far=4.0)])
    return _t(poses, dev), torch.from_numpy(R.k_inv(VH, VW, 0.09)), VH, VW


def _by_hand(pkg, model, dev, views, col0, min_opacity, trunc=None):
    """render(maps=True) per view, the depth rule in torch, tsdf_integrate"""
    pb, K, H, W = views
    row = torch.arange(H, device=dev).repeat_interleave(W)
    col = torch.arange(W, device=dev).repeat(H)
    D, A = [], []
    for c in range(pb.shape[0]):
        M = model.render(row, col, pb[c].expand(H * W, 17), K, maps=True)[2]
        d, a = M[:, col0], M[:, col0 + 1]
        D.append(torch.where(a >= min_opacity, d / a, torch.full_like(d, float("inf"))).view(H, W))
        A.append(a.view(H, W))
    D, A = torch.stack(D), torch.stack(A)
    lo32, hi32 = np.asarray(LO, F32), np.asarray(HI, F32)
    T, Wt = pkg.mesh.tsdf_volume(RES, dev)
    pkg.mesh.tsdf_integrate(T, Wt, lo32, pkg.nerf.grid_step(lo32, hi32, (RES,) * 3), D, pb, K, opacity=A, trunc=trunc, min_opacity=min_opacity)
    return T, Wt, A


def test_fuse_depth_plumbing(pkg, dev, model):
    views = _views(dev)
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    try:
        for kind, col0 in (("coarse", 0), ("fine", 2)):
            T, Wt, A = _by_hand(pkg, model, dev, views, col0, 0.5)
            mid = float(A.median())  # a threshold that leaves foreground and background pixels
            for mo in (0.5, mid):
                T, Wt, A = _by_hand(pkg, model, dev, views, col0, mo)
                got = model.fuse_depth(views, LO, HI, RES, depth=kind, min_opacity=mo)
                one = model.fuse_depth(views, LO, HI, RES, depth=kind, min_opacity=mo, views_per_call=1)
                print(f"{kind}, min_opacity {mo:.3g}: {int((A >= mo).sum())} of {A.numel()} pixels foreground, {int((Wt > 0).sum())} of {Wt.numel()} "
                      f"voxels observed, T in [{float(T.min()):.3f}, {float(T.max()):.3f}]")
                assert eq(got[0], T) and eq(got[1], Wt) and eq(one[0], T) and eq(one[1], Wt) and int((Wt > 0).sum()) > 0
            assert (A >= mid).any() and (A < mid).any()
        mid_c = float(_by_hand(pkg, model, dev, views, 0, 0.5)[2].median())
        auto = model.fuse_depth(views, LO, HI, RES, min_opacity=mid_c)
        coarse = model.fuse_depth(views, LO, HI, RES, depth="coarse", min_opacity=mid_c)
        assert not model.corrected and eq(auto[0], coarse[0]) and eq(auto[1], coarse[1])
        model.corrected = True
        auto = model.fuse_depth(views, LO, HI, RES, min_opacity=mid_c)
        fine = model.fuse_depth(views, LO, HI, RES, depth="fine", min_opacity=mid_c)
        hand = _by_hand(pkg, model, dev, views, 2, mid_c)
        assert eq(auto[0], fine[0]) and eq(auto[1], fine[1]) and eq(auto[0], hand[0]) and eq(auto[1], hand[1])
    finally:
        model.corrected = False
    with pytest.raises(ValueError, match="depth="):
        model.fuse_depth(views, LO, HI, RES, depth="median")
    empty = model.fuse_depth((views[0][:0], views[1], VH, VW), LO, HI, RES)
    assert not empty[0].any() and not empty[1].any()


def test_extract_mesh_tsdf_is_the_shared_stages_by_hand(pkg, dev, model):
    views = _views(dev)
    mid = float(_by_hand(pkg, model, dev, views, 0, 0.5)[2].median())
    lo32, hi32, shape = np.asarray(LO, F32), np.asarray(HI, F32), (RES,) * 3
    for kw in (dict(color=True, normals="grid"), dict(color=True, normals="field", min_faces=1), dict(color=False, normals="grid", smooth=1, simplify=2)):
        got = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, **kw)
        T, Wt = model.fuse_depth(views, LO, HI, RES, min_opacity=mid)
        assert torch.equal(model.last_tsdf[0], T) and torch.equal(model.last_tsdf[1], Wt)
        v, f, n = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt), 0.0, lo32, pkg.nerf.grid_step(lo32, hi32, shape))
        full = dict(color=True, normals="grid", min_faces=None, keep_largest=None, simplify=None, smooth=None, visible=None)
        full.update(kw)
        want = model._mesh_stages(v, f, n, lo32, hi32, shape, **full)
        print(f"extract_mesh_tsdf {kw}: V {len(got.verts)} F {len(got.faces)} (marching cubes: V {len(v)} F {len(f)})")
        assert len(v) > 0
        for a, b in zip(got, want):
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))))
    with pytest.raises(ValueError, match="normals"):
        model.extract_mesh_tsdf(views, LO, HI, RES, normals="faces")


# ---- (6) refusals on the host: nothing is enqueued ----

def test_host_refusals_leave_the_volumes_untouched(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    f3 = pkg._abi.f32_array
    nx, ny, nz, n, H, W = 4, 5, 6, 2, 3, 4
    T = torch.full((nx, ny, nz), 0.25, device=dev)
    Wt = torch.full((nx, ny, nz), 3.0, device=dev)
    depth = torch.full((n, H, W), 2.0, device=dev)
    opac = torch.ones(n, H, W, device=dev)
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    dbl = lambda v: (ctypes.c_double * len(v))(*v)

    def call(tp=T.data_ptr(), wp=Wt.data_ptr(), shape=(nx, ny, nz), lo=f3([-1, -1, -1]), step=f3([0.5, 0.5, 0.5]), dp=depth.data_ptr(),
             op=opac.data_ptr(), n=n, H=H, W=W, cam=f3([0, 0, -3] * 2), Q=dbl(eye * 2), trunc=1.0, mo=0.5, flags=1):
        return L.nerf_hip_tsdf_integrate(tp, wp, *shape, lo, step, dp, op, n, H, W, cam, Q, trunc, mo, flags, st)

    bad = [dict(shape=(0, ny, nz)), dict(shape=(nx, -1, nz)), dict(shape=(2048, 1024, 1024)), dict(n=-1), dict(H=0), dict(W=0), dict(W=-3),
           dict(n=1, H=65536, W=32768), dict(n=1 << 20, H=1 << 30, W=1 << 30), dict(n=1 << 30, H=4, W=4), dict(tp=None), dict(wp=None), dict(lo=None), dict(step=None), dict(dp=None), dict(cam=None), dict(Q=None),
           dict(lo=f3([-1, nan, -1])), dict(lo=f3([inf, -1, -1])), dict(step=f3([0.5, 0.5, inf])), dict(step=f3([nan, 0.5, 0.5])),
           dict(cam=f3([0, 0, -3, 0, nan, -3])), dict(cam=f3([-inf, 0, -3, 0, 0, -3])), dict(Q=dbl(eye + [1.0, 0, 0, 0, inf, 0, 0, 0, 1.0])),
           dict(Q=dbl([nan] + eye[1:] + eye)), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan), dict(trunc=inf), dict(mo=nan), dict(flags=2),
           dict(flags=3), dict(flags=-1)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, kw
        with pytest.raises(pkg._abi.NerfHipError):
            pkg._abi.check(rc)
    torch.cuda.synchronize()
    assert (T == 0.25).all() and (Wt == 3.0).all()
    # no views: a no-op, whatever the image pointers are
    assert call(n=0) == 0 and call(n=0, dp=None, op=None, cam=None, Q=None) == 0
    torch.cuda.synchronize()
    assert (T == 0.25).all() and (Wt == 3.0).all()
    # and the good call goes through, with and without the opacity, infinite min_opacity included (every pixel background)
    assert call() == 0 and call(op=None, flags=0) == 0 and call(mo=inf) == 0 and call(mo=-inf) == 0
    torch.cuda.synchronize()
    assert (Wt >= 3.0).all() and (Wt > 3.0).any()
    # the Python layer: CPU tensors and mismatched shapes raise before the library is asked
    with pytest.raises(ValueError, match="poses"):
        pkg.mesh.tsdf_integrate(T, Wt, (-1, -1, -1), (0.5, 0.5, 0.5), depth, np.zeros((3, 17), F32), torch.eye(3), trunc=1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_integrate(T.cpu(), Wt.cpu(), (-1, -1, -1), (0.5, 0.5, 0.5), depth, np.zeros((2, 17), F32), torch.eye(3), trunc=1.0)


# ---- (7) the runner ----

def test_runner_tsdf_from(pkg, dev, tmp_path, capsys):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    level = float(np.median(run.density_grid(16, save=False)))
    capsys.readouterr()
    plain = run.extract_mesh(16, level, save=True)
    out_before = capsys.readouterr().out
    files = glob.glob(rs + "*.ply")
    assert len(files) == 1 and files[0].endswith("_mesh16.ply") and "[TSDF]" not in out_before
    before = open(files[0], "rb").read()
    got = run.extract_mesh(16, level, save=True, tsdf_from="train", tsdf_every=2)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH]") and "[TSDF]" in ln]
    tsdf_files = glob.glob(rs + "*_mesh16_tsdf.ply")
    assert len(line) == 1 and len(tsdf_files) == 1 and sorted(glob.glob(rs + "*.ply")) == sorted(files + tsdf_files)
    T, Wt = run.model.last_tsdf
    assert f"2 train views fused, {int((Wt > 0).sum())} / {16 ** 3} lattice points observed" in line[0] and "ignored" in line[0]
    want = run.model.extract_mesh_tsdf((run.train_rays.poses[::2], run.K_inv, 24, 24), (-1.5,) * 3, (1.5,) * 3, 16)
    assert np.array_equal(got.verts, want.verts.cpu().numpy()) and np.array_equal(got.faces, want.faces.cpu().numpy())
    v, f, _, _ = pkg.mesh.read_ply(tsdf_files[0])
    assert np.array_equal(v, got.verts) and np.array_equal(f, got.faces)
    # without the argument: what it printed and wrote before
    again = run.extract_mesh(16, level, save=True)
    assert capsys.readouterr().out == out_before and open(files[0], "rb").read() == before and np.array_equal(again.faces, plain.faces)
    assert sorted(glob.glob(rs + "*.ply")) == sorted(files + tsdf_files)
    with pytest.raises(ValueError, match="tsdf_from"):
        run.extract_mesh(16, level, save=False, tsdf_from="all")
    with pytest.raises(ValueError, match="tsdf_every"):
        run.extract_mesh(16, level, save=False, tsdf_from="val", tsdf_every=0)
