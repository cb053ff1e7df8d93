"""GPU: colour fusion on the device (nerf_hip_tsdf_integrate_color / nerf_hip_tsdf_sample_color; mesh.tsdf_color_volume /
tsdf_integrate(rgb=, color=) / tsdf_sample_color; NeRFModel.fuse_depth(color=) / extract_mesh_tsdf(color="fused", unseen="skip");
NeRFRunner.extract_mesh(tsdf_color=, tsdf_unseen=)) against the numpy restatements of rules TC and S in tests/tsdf_color_reference.py.
Volumes and colours are compared as bits."""
import ctypes
import glob

import numpy as np
import pytest
import torch

import tsdf_color_reference as RC
import tsdf_reference as R
from conftest import load_golden
from test_tsdf_color_cpu import sample_points

pytestmark = pytest.mark.gpu
F32 = np.float32


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the scenes are read-only)


def _same(got, want):
    """a device fp32 tensor and a numpy fp32 array, bit for bit"""
    want = np.array(want, F32)  # (a copy: the scenes are read-only)
    return got.dtype == torch.float32 and tuple(got.shape) == want.shape and torch.equal(got.cpu().contiguous().view(torch.int32),
                                                                                         torch.from_numpy(want).view(torch.int32))


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _fuse(pkg, dev, s, rgb, state=None, views=slice(None), opacity=True, **kw):
    T, Wt, C = state if state is not None else (*pkg.mesh.tsdf_volume(s["shape"], dev), pkg.mesh.tsdf_color_volume(s["shape"], dev))
    return pkg.mesh.tsdf_integrate(T, Wt, s["lo"], s["step"], _t(s["depth"][views], dev), np.ascontiguousarray(s["poses"][views]), s["K"],
                                   opacity=_t(s["opacity"][views], dev) if opacity else None, trunc=s["trunc"], rgb=_t(rgb[views], dev), color=C, **kw)


def _plain(pkg, dev, s, views=slice(None), opacity=True, **kw):
    T, Wt = pkg.mesh.tsdf_volume(s["shape"], dev)
    return pkg.mesh.tsdf_integrate(T, Wt, s["lo"], s["step"], _t(s["depth"][views], dev), np.ascontiguousarray(s["poses"][views]), s["K"],
                                   opacity=_t(s["opacity"][views], dev) if opacity else None, trunc=s["trunc"], **kw)


# ---- (1) rule TC bit for bit, on one partial workgroup and on four ----

@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 10, 11)])
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("with_opacity", [True, False])
def test_random_case_bit_identical(pkg, dev, shape, carve, with_opacity):
    s = R.random_case(shape=shape)  # 3 cameras, 8 x 12 images
    rgb = RC.random_rgb(s)
    assert np.isnan(rgb).any() and np.isinf(rgb).any()
    z, zc = np.zeros(shape, F32), np.zeros(shape + (4,), F32)
    op = s["opacity"] if with_opacity else None
    want = RC.integrate_color(z, z, zc, s["lo"], s["step"], s["depth"], op, rgb, s["cams"], s["trunc"], 0.5, carve)
    T, Wt, C = _fuse(pkg, dev, s, rgb, opacity=with_opacity, carve=carve)
    assert tuple(C.shape) == shape + (4,) and _same(T, want[0]) and _same(Wt, want[1]) and _same(C, want[2])
    assert (want[2][..., 3] > 0).any() and (want[2][..., 3] >= 2).any() and (want[2][..., 3] < want[1]).any()
    plain = _plain(pkg, dev, s, opacity=with_opacity, carve=carve)
    assert _eq(T, plain[0]) and _eq(Wt, plain[1])  # the geometry is nerf_hip_tsdf_integrate's
    # a second call continues from the state the first left (the views in reverse order)
    rev = slice(None, None, -1)
    want2 = RC.integrate_color(*want, s["lo"], s["step"], s["depth"][rev], None if op is None else op[rev], rgb[rev], s["cams"][rev], s["trunc"], 0.5, carve)
    out = _fuse(pkg, dev, s, rgb, (T, Wt, C), views=rev, opacity=with_opacity, carve=carve)
    assert out[2] is C and _same(T, want2[0]) and _same(Wt, want2[1]) and _same(C, want2[2])


# ---- (2) the grouping of the views into launches and calls changes nothing ----

def test_grouping_into_launches_and_calls(pkg, dev):
    n = 2 * pkg._abi.TSDF_VIEWS_PER_LAUNCH + 1
    s = R.random_case(n=n, H=4, W=6, seed=1)
    rgb = RC.random_rgb(s)
    z = np.zeros(s["shape"], F32)
    want = RC.integrate_color(z, z, np.zeros(s["shape"] + (4,), F32), s["lo"], s["step"], s["depth"], s["opacity"], rgb, s["cams"], s["trunc"], 0.5, True)
    assert want[2][..., 3].max() > 2
    got = _fuse(pkg, dev, s, rgb)
    assert all(_same(a, b) for a, b in zip(got, want))
    state = (*pkg.mesh.tsdf_volume(s["shape"], dev), pkg.mesh.tsdf_color_volume(s["shape"], dev))
    for c in range(n):
        _fuse(pkg, dev, s, rgb, state, views=slice(c, c + 1))
    assert all(_same(a, b) for a, b in zip(state, want))


# ---- (3) cameras inside the lattice, on a lattice point, and with a frame that covers a part of it ----

def test_edge_cameras(pkg, dev):
    s = dict(R.random_case())
    P = R.lattice(s["lo"], s["step"], s["shape"])
    H, W = s["H"], s["W"]
    at_point = P[2, 3, 3]
    poses = np.stack([R.look_at((0.1, 0.05, -0.2), (1.0, 0.2, -0.1)), R.look_at(at_point.astype(np.float64), (1.0, 1.0, 1.0)),
                      R.look_at((0.0, -3.0, 0.2), (0.3, 0.0, 0.2))])
    poses[1, [3, 8, 13]] = at_point
    Ks = [R.k_inv(H, W, 0.3), R.k_inv(H, W, 0.3), R.k_inv(H, W, 0.06)]
    depths = [np.full((1, H, W), d, F32) for d in (3.25, 3.25, 5.2)]  # far enough that some observed voxels lie beyond trunc in front
    rgb = np.random.default_rng(9).random((1, H, W, 3)).astype(F32)
    z, zc = np.zeros(s["shape"], F32), np.zeros(s["shape"] + (4,), F32)
    total = (z, z, zc)
    state = (*pkg.mesh.tsdf_volume(s["shape"], dev), pkg.mesh.tsdf_color_volume(s["shape"], dev))
    for c in range(3):
        cams, depth = [R.camera_q(poses[c], Ks[c])], depths[c]
        one = RC.integrate_color(z, z, zc, s["lo"], s["step"], depth, None, rgb, cams, s["trunc"], 0.5, True)
        col = one[2][..., 3] > 0
        print(f"camera {c}: {int((one[1] > 0).sum())} of {col.size} voxels observed, {int(col.sum())} with a colour")
        assert 0 < col.sum() < (one[1] > 0).sum()
        assert not (col & ~(one[1] > 0)).any() and not one[2][~col].any()  # no colour without a geometry observation
        got = pkg.mesh.tsdf_integrate(*pkg.mesh.tsdf_volume(s["shape"], dev), s["lo"], s["step"], _t(depth, dev), poses[c:c + 1], Ks[c],
                                      trunc=s["trunc"], rgb=_t(rgb, dev), color=pkg.mesh.tsdf_color_volume(s["shape"], dev))
        assert all(_same(a, b) for a, b in zip(got, one))
        total = RC.integrate_color(*total, s["lo"], s["step"], depth, None, rgb, cams, s["trunc"], 0.5, True)
        pkg.mesh.tsdf_integrate(state[0], state[1], s["lo"], s["step"], _t(depth, dev), poses[c:c + 1], Ks[c], trunc=s["trunc"], rgb=_t(rgb, dev),
                                color=state[2])
    assert all(_same(a, b) for a, b in zip(state, total))
    none = total[1] == 0
    assert none.any() and not state[2].cpu().numpy()[none].any()  # what no view observes keeps a zero colour state


# ---- (4) rule S bit for bit ----

@pytest.mark.parametrize("shape", [(5, 6, 7), (1, 6, 7)])
def test_sample_color_bit_identical(pkg, dev, shape):
    C = RC.random_color_volume(shape)
    assert 0.25 < (C[..., 3] == 0).mean() < 0.55
    lo, step = np.array([-1.0, -0.9, -1.1], F32), np.array([0.5, 0.36, 0.37], F32)
    pts = sample_points(shape, lo, step)
    if shape[0] > 1:  # a cell whose eight corners are all empty, and points inside it
        C[1:3, 2:4, 3:5, 3] = 0
        P = R.lattice(lo, step, shape)
        pts[540:560] = P[1, 2, 3] + np.random.default_rng(4).uniform(0.05, 0.95, (20, 3)).astype(F32) * step
    want_rgb, want_valid = RC.sample_color(C, lo, step, pts)
    rgb, valid = pkg.mesh.tsdf_sample_color(_t(C, dev), lo, step, _t(pts, dev))
    assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), want_valid) and _same(rgb, want_rgb)
    assert want_valid.any() and (~want_valid).any() and not want_rgb[~want_valid].any()
    if shape[0] > 1:
        assert not want_valid[540:560].any()
    assert not want_valid[500:530].any()  # NaN and inf coordinates
    again = pkg.mesh.tsdf_sample_color(_t(C, dev), lo, step, _t(pts, dev))
    assert _eq(again[0], rgb) and torch.equal(again[1], valid)
    empty = pkg.mesh.tsdf_sample_color(_t(C, dev), lo, step, torch.empty(0, 3, device=dev))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,)


def test_sphere_colours_on_the_device(pkg, dev):
    s = R.sphere_scene()
    want = RC.sphere_fused_color(True)
    got = _fuse(pkg, dev, s, RC.sphere_rgb())
    assert all(_same(a, b) for a, b in zip(got, want))
    T, Wt, C = got
    v, f, n = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt, "empty"), 0.0, s["lo"], s["step"], valid=Wt > 0)
    solid = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt, "solid"), 0.0, s["lo"], s["step"])
    assert len(v) == 1024 and _eq(v, solid[0]) and _eq(f, solid[1])
    rgb, valid = pkg.mesh.tsdf_sample_color(C, s["lo"], s["step"], v)
    p = v.double().cpu().numpy()
    err = np.abs(rgb.double().cpu().numpy() - (0.5 + 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True)))
    print(f"sphere: worst channel error of the fused colours {err.max():.4f}, mean {err.mean():.4f}")
    assert bool(valid.all()) and err.max() < 0.10


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


def _by_hand(pkg, model, dev, views, min_opacity):
    """render(maps=True) per view, the depth rule in torch, C_fine as the colour image, tsdf_integrate(rgb=, color=)"""
    pb, K, H, W = views
    row = torch.arange(H, device=dev).repeat_interleave(W)
    col = torch.arange(W, device=dev).repeat(H)
    D, A, RGB = [], [], []
    for c in range(pb.shape[0]):
        _, Cf, M = model.render(row, col, pb[c].expand(H * W, 17), K, maps=True)
        d, a = M[:, 0], M[:, 1]
        D.append(torch.where(a >= min_opacity, d / a, torch.full_like(d, float("inf"))).view(H, W))
        A.append(a.view(H, W))
        RGB.append(Cf.view(H, W, 3))
    D, A, RGB = torch.stack(D), torch.stack(A), torch.stack(RGB)
    lo32, hi32 = np.asarray(LO, F32), np.asarray(HI, F32)
    T, Wt = pkg.mesh.tsdf_volume(RES, dev)
    C = pkg.mesh.tsdf_color_volume(RES, dev)
    pkg.mesh.tsdf_integrate(T, Wt, lo32, pkg.nerf.grid_step(lo32, hi32, (RES,) * 3), D, pb, K, opacity=A, min_opacity=min_opacity, rgb=RGB, color=C)
    return T, Wt, C, A


def test_fuse_depth_color_plumbing(pkg, dev, model):
    views = _views(dev)
    mid = float(_by_hand(pkg, model, dev, views, 0.5)[3].median())
    T, Wt, C, _ = _by_hand(pkg, model, dev, views, mid)
    got = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, color=True)
    one = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, color=True, views_per_call=1)
    plain = model.fuse_depth(views, LO, HI, RES, min_opacity=mid)
    print(f"fuse_depth(color=True): {int((Wt > 0).sum())} of {Wt.numel()} voxels observed, {int((C[..., 3] > 0).sum())} with a colour")
    assert len(got) == 3 and len(plain) == 2 and int((C[..., 3] > 0).sum()) > 0
    assert all(_eq(a, b) for a, b in zip(got, (T, Wt, C))) and all(_eq(a, b) for a, b in zip(one, (T, Wt, C)))
    assert _eq(plain[0], T) and _eq(plain[1], Wt)
    empty = model.fuse_depth((views[0][:0], views[1], VH, VW), LO, HI, RES, color=True)
    assert len(empty) == 3 and tuple(empty[2].shape) == (RES, RES, RES, 4) and not empty[2].any()


def test_extract_mesh_tsdf_fused_skip_is_the_stages_by_hand(pkg, dev, model):
    views = _views(dev)
    mid = float(_by_hand(pkg, model, dev, views, 0.5)[3].median())
    lo32, hi32, shape = np.asarray(LO, F32), np.asarray(HI, F32), (RES,) * 3
    step = pkg.nerf.grid_step(lo32, hi32, shape)
    got = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, color="fused", unseen="skip")
    T, Wt, C = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, color=True)
    assert len(model.last_tsdf) == 3 and all(_eq(a, b) for a, b in zip(model.last_tsdf, (T, Wt, C)))
    v, f, n = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt, "empty"), 0.0, lo32, step, valid=Wt > 0)
    rgb, ok = pkg.mesh.tsdf_sample_color(C, lo32, step, v)
    field = model.query(v, -n)[0]
    want_rgb = torch.where(ok[:, None], rgb, field)
    print(f"fused + skip: V {len(v)} F {len(f)}, {int(ok.sum())} vertices with a fused colour, {int((~ok).sum())} from the field")
    assert len(v) > 0 and model.last_fused_fallback == int((~ok).sum())
    assert _eq(got.verts, v) and _eq(got.faces, f) and _eq(got.normals, n) and _eq(got.rgb, want_rgb)
    # fused colours through the later stages: sampled at the final vertices
    got2 = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, color="fused", smooth=1)
    v2, f2, n2 = pkg.mesh.marching_cubes(pkg.mesh.tsdf_grid(T, Wt), 0.0, lo32, step)
    st = model._mesh_stages(v2, f2, n2, lo32, hi32, shape, False, "grid", None, None, None, 1, None)
    rgb2, ok2 = pkg.mesh.tsdf_sample_color(C, lo32, step, st.verts)
    want2 = torch.where(ok2[:, None], rgb2, model.query(st.verts, -st.normals)[0])
    assert _eq(got2.verts, st.verts) and _eq(got2.rgb, want2)
    # the fall-back: a volume without any colour sends every vertex to the field, one with half its colours removed the vertices there
    plain = model._mesh_stages(v2, f2, n2, lo32, hi32, shape, True, "grid", None, None, None, None, None)
    none = model._mesh_stages(v2, f2, n2, lo32, hi32, shape, True, "grid", None, None, None, None, None, fused=torch.zeros_like(C))
    assert model.last_fused_fallback == len(v2) > 0 and _eq(none.rgb, plain.rgb)
    half = C.clone()
    half[: RES // 2, :, :, 3] = 0
    some = model._mesh_stages(v2, f2, n2, lo32, hi32, shape, True, "grid", None, None, None, None, None, fused=half)
    rgb3, ok3 = pkg.mesh.tsdf_sample_color(half, lo32, step, v2)
    print(f"half the colours removed: {int(ok3.sum())} of {len(v2)} vertices keep a fused colour, {model.last_fused_fallback} fall back")
    assert model.last_fused_fallback == int((~ok3).sum()) and _eq(some.rgb, torch.where(ok3[:, None], rgb3, plain.rgb))
    # today's keywords give today's bits
    old = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, color=True, unseen="solid")
    T0, Wt0 = model.last_tsdf
    assert _eq(T0, T) and _eq(Wt0, Wt)
    want = model._mesh_stages(v2, f2, n2, lo32, hi32, shape, True, "grid", None, None, None, None, None)
    assert all(_eq(a, b) for a, b in zip(old, want))
    with pytest.raises(ValueError, match="unseen"):
        model.extract_mesh_tsdf(views, LO, HI, RES, unseen="open")
    with pytest.raises(ValueError, match="color"):
        model.extract_mesh_tsdf(views, LO, HI, RES, color="views")


# ---- (6) refusals on the host: nothing is enqueued ----

def test_host_refusals_leave_the_volumes_untouched(pkg, dev):
    L, st = pkg._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    f3 = pkg._abi.f32_array
    nx, ny, nz, n, H, W = 4, 5, 6, 2, 3, 4
    T = torch.full((nx, ny, nz), 0.25, device=dev)
    Wt = torch.full((nx, ny, nz), 3.0, device=dev)
    C = torch.full((nx, ny, nz, 4), 0.5, device=dev)
    depth = torch.full((n, H, W), 2.0, device=dev)
    opac = torch.ones(n, H, W, device=dev)
    rgb = torch.full((n, H, W, 3), 0.75, device=dev)
    nan, inf = float("nan"), float("inf")
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    dbl = lambda v: (ctypes.c_double * len(v))(*v)

    def call(tp=T.data_ptr(), wp=Wt.data_ptr(), cp=C.data_ptr(), shape=(nx, ny, nz), lo=f3([-1, -1, -1]), step=f3([0.5, 0.5, 0.5]),
             dp=depth.data_ptr(), op=opac.data_ptr(), rp=rgb.data_ptr(), n=n, H=H, W=W, cam=f3([0, 0, -3] * 2), Q=dbl(eye * 2), trunc=1.0, mo=0.5,
             flags=1):
        return L.nerf_hip_tsdf_integrate_color(tp, wp, cp, *shape, lo, step, dp, op, rp, n, H, W, cam, Q, trunc, mo, flags, st)

    bad = [dict(cp=None), dict(rp=None), dict(cp=C.data_ptr() + 4),
           dict(shape=(0, ny, nz)), dict(shape=(nx, -1, nz)), dict(shape=(2048, 1024, 1024)), dict(n=-1), dict(H=0), dict(W=0), dict(W=-3),
           dict(n=1, H=65536, W=32768), dict(n=1 << 30, H=4, W=4), dict(tp=None), dict(wp=None), dict(lo=None), dict(step=None), dict(dp=None),
           dict(cam=None), dict(Q=None), dict(lo=f3([-1, nan, -1])), dict(lo=f3([inf, -1, -1])), dict(step=f3([0.5, 0.5, inf])),
           dict(step=f3([nan, 0.5, 0.5])), dict(cam=f3([0, 0, -3, 0, nan, -3])), dict(cam=f3([-inf, 0, -3, 0, 0, -3])),
           dict(Q=dbl(eye + [1.0, 0, 0, 0, inf, 0, 0, 0, 1.0])), dict(Q=dbl([nan] + eye[1:] + eye)), dict(trunc=0.0), dict(trunc=-1.0),
           dict(trunc=nan), dict(trunc=inf), dict(mo=nan), dict(flags=2), dict(flags=3), dict(flags=-1)]
    for kw in bad:
        rc = call(**kw)
        assert rc == -1, kw
        with pytest.raises(pkg._abi.NerfHipError):
            pkg._abi.check(rc)
    torch.cuda.synchronize()
    assert (T == 0.25).all() and (Wt == 3.0).all() and (C == 0.5).all()
    # no views: a no-op, whatever the image pointers are -- but the colour volume is still required
    assert call(n=0) == 0 and call(n=0, dp=None, op=None, rp=None, cam=None, Q=None) == 0 and call(n=0, cp=None) == -1
    torch.cuda.synchronize()
    assert (T == 0.25).all() and (Wt == 3.0).all() and (C == 0.5).all()
    # the sampler's refusals leave its outputs untouched
    pts = torch.zeros(5, 3, device=dev)
    out = torch.full((5, 3), 9.0, device=dev)
    ok = torch.full((5,), 7, dtype=torch.uint8, device=dev)

    def sample(cp=C.data_ptr(), shape=(nx, ny, nz), lo=f3([-1, -1, -1]), step=f3([0.5, 0.5, 0.5]), pp=pts.data_ptr(), M=5, rp=out.data_ptr(),
               vp=ok.data_ptr()):
        return L.nerf_hip_tsdf_sample_color(cp, *shape, lo, step, pp, M, rp, vp, st)

    for kw in (dict(cp=None), dict(cp=C.data_ptr() + 8), dict(shape=(0, ny, nz)), dict(shape=(2048, 1024, 1024)), dict(M=-1), dict(M=1 << 31),
               dict(lo=None), dict(step=None), dict(lo=f3([nan, -1, -1])), dict(step=f3([0.5, 0.0, 0.5])), dict(step=f3([0.5, 0.5, -1])),
               dict(step=f3([inf, 0.5, 0.5])), dict(pp=None), dict(rp=None), dict(vp=None)):
        assert sample(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out == 9.0).all() and (ok == 7).all()
    assert sample(M=0, pp=None, rp=None, vp=None) == 0 and sample(shape=(1, ny, nz), step=f3([0.0, 0.5, 0.5])) == 0
    # and the good calls go through
    assert call() == 0 and call(op=None, flags=0) == 0 and sample() == 0
    torch.cuda.synchronize()
    assert (Wt > 3.0).any() and (C[..., 3] > 0.5).any() and (ok <= 1).all()
    # the Python layer: half a pair, CPU tensors and mismatched shapes raise before the library is asked
    poses = np.stack([R.look_at((0, 0, -3), (0, 0, 0)), R.look_at((3, 0, 0), (0, 0, 0))])
    args = (T, Wt, (-1, -1, -1), (0.5, 0.5, 0.5), depth, poses, torch.eye(3))
    with pytest.raises(ValueError, match="both"):
        pkg.mesh.tsdf_integrate(*args, trunc=1.0, rgb=rgb)
    with pytest.raises(ValueError, match="both"):
        pkg.mesh.tsdf_integrate(*args, trunc=1.0, color=C)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_integrate(*args, trunc=1.0, rgb=rgb, color=C.cpu())
    with pytest.raises(ValueError, match="rgb"):
        pkg.mesh.tsdf_integrate(*args, trunc=1.0, rgb=rgb[:, :, :, :2], color=C)
    with pytest.raises(ValueError, match="color"):
        pkg.mesh.tsdf_integrate(*args, trunc=1.0, rgb=rgb, color=C[..., :3].contiguous())
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_sample_color(C.cpu(), (-1, -1, -1), (0.5, 0.5, 0.5), pts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pkg.mesh.tsdf_color_volume(4, "cpu")


# ---- (7) the runner ----

def test_runner_tsdf_color_and_unseen(pkg, dev, tmp_path, capsys):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    capsys.readouterr()
    plain = run.extract_mesh(16, 0.0, save=True, tsdf_from="train", tsdf_every=2)
    out_before = capsys.readouterr().out
    files = glob.glob(rs + "*.ply")
    assert len(files) == 1 and files[0].endswith("_mesh16_tsdf.ply") and "colour" not in out_before and len(run.model.last_tsdf) == 2
    before = open(files[0], "rb").read()
    got = run.extract_mesh(16, 0.0, save=True, tsdf_from="train", tsdf_every=2, tsdf_color=True, tsdf_unseen="skip")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH]") and "[TSDF]" in ln]
    new = glob.glob(rs + "*_mesh16_tsdf_fused_skip.ply")
    assert len(line) == 1 and len(new) == 1 and sorted(glob.glob(rs + "*.ply")) == sorted(files + new)
    T, Wt, C = run.model.last_tsdf
    assert (f"{int((Wt > 0).sum())} / {16 ** 3} lattice points observed" in line[0]
            and f"{int((C[..., 3] > 0).sum())} lattice points with a colour, {run.model.last_fused_fallback} vertices coloured by the field" in line[0])
    want = run.model.extract_mesh_tsdf((run.train_rays.poses[::2], run.K_inv, 24, 24), (-1.5,) * 3, (1.5,) * 3, 16, color="fused", unseen="skip")
    assert np.array_equal(got.verts, want.verts.cpu().numpy()) and np.array_equal(got.faces, want.faces.cpu().numpy())
    assert np.array_equal(got.rgb.view(np.int32), want.rgb.cpu().numpy().view(np.int32))
    print(f"runner: V {len(got.verts)} F {len(got.faces)}; {line[0]}")
    v, f, _, c = pkg.mesh.read_ply(new[0])
    assert np.array_equal(v, got.verts) and np.array_equal(f, got.faces)
    assert c is not None and np.array_equal(c, np.clip(np.rint(got.rgb.astype(np.float64) * 255), 0, 255).astype(np.uint8))
    # one flag alone
    skip = run.extract_mesh(16, 0.0, save=True, tsdf_from="train", tsdf_every=2, tsdf_unseen="skip")
    skip_line = [ln for ln in capsys.readouterr().out.splitlines() if "[TSDF]" in ln]
    assert len(glob.glob(rs + "*_mesh16_tsdf_skip.ply")) == 1 and np.array_equal(skip.verts, got.verts)
    assert f"0 lattice points with a colour, {len(skip.verts)} vertices coloured by the field" in skip_line[0]  # no fusion: all from the field
    # without the new arguments: what it printed and wrote before
    again = run.extract_mesh(16, 0.0, save=True, tsdf_from="train", tsdf_every=2)
    assert capsys.readouterr().out == out_before and open(files[0], "rb").read() == before and np.array_equal(again.faces, plain.faces)
    with pytest.raises(ValueError, match="tsdf_unseen"):
        run.extract_mesh(16, 0.0, save=False, tsdf_from="val", tsdf_unseen="open")
