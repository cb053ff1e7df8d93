"""GPU: point gradients of the field (NeRFModel.query_grad / field, nerf_hip_query_grad) -- a hand-built field with
a closed-form gradient, the fp64 autograd reference built from the oracle, bit-identity with query(), determinism, autograd through
model.field, and analytic mesh normals."""
import glob
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_mesh_cpu import _read_ply

pytestmark = pytest.mark.gpu
CHUNK = 256 * 4 * 32 * 4  # kernels.h QGRAD_CHUNK


def _model(pkg, oracle, dev, w):
    m = pkg.NeRFModel(64, 128, 8)
    m.load_state_dict(w)
    return m.to(dev)


def _unit_dirs(gen, M):
    d = torch.randn(M, 3, generator=gen)
    return d / d.norm(dim=1, keepdim=True)


def _sine_weights(oracle):
    """sigma = |sin(f_0 x)|: h_0[0] = relu(gamma_p[0] + 2) = sin(phi) + 2 carried through layers 1..7 by unit weights (column 0 of W4's
    hidden part), w_sigma[0] = 1, b_sigma = -2; every other weight 0."""
    w = OrderedDict((k, torch.zeros(s)) for k, s in oracle.PARAM_SHAPES.items())
    w["network.point_layer.0.0.weight"][0, 0] = 1.0
    w["network.point_layer.0.0.bias"][0] = 2.0
    for i in range(1, 8):
        w[f"network.point_layer.{i}.0.weight"][0, 0] = 1.0
    w["network.sigma_layer.0.weight"][0, 0] = 1.0
    w["network.sigma_layer.0.bias"][0] = -2.0
    return w


def test_analytic_field_gradient_and_normals(oracle, pkg, dev):
    w = _sine_weights(oracle)
    m = _model(pkg, oracle, dev, w)
    f0 = float(oracle.frequencies()[0][0])
    gen = torch.Generator().manual_seed(7)
    pts = (torch.rand(20000, 3, generator=gen) * 8.0 - 4.0).float()
    _, sig, dp = m.query_grad(pts.to(dev))
    phi = (pts[:, 0] * oracle.frequencies()[0][0]).double()  # fp32(x * f_0)
    s, c = torch.sin(phi), torch.cos(phi)
    keep = s.abs() >= 1e-6  # the fp32 round trip through the +2 / -2 biases can leave spre = 0 next to a zero of sin
    want = torch.sign(s) * f0 * c
    dp = dp.cpu().double()
    assert keep.sum() > 19000
    assert (dp[keep, 0] - want[keep]).abs().max() <= 1e-6 * f0
    assert torch.equal(dp[:, 1:], torch.zeros_like(dp[:, 1:]))
    assert (sig.cpu().double() - s.abs()).abs().max() < 1e-6
    # analytic normals of the planes |sin(pi x)| = 0.5: -g / |g| = (+-1, 0, 0), whatever the grid spacing
    mesh = m.extract_mesh((-1.0, -0.5, -0.5), (1.0, 0.5, 0.5), (41, 9, 9), 0.5, color=False, normals="field")
    n = mesh.normals.cpu().double()
    assert len(n) > 100
    assert (n[:, 0].abs() - 1.0).abs().max() <= 1e-6 and n[:, 1:].abs().max() <= 1e-6
    # outward = toward decreasing sigma: the same side the grid normals point to
    grid = m.extract_mesh((-1.0, -0.5, -0.5), (1.0, 0.5, 0.5), (41, 9, 9), 0.5, color=False)
    assert torch.equal(grid.verts, mesh.verts) and torch.equal(torch.sign(grid.normals[:, 0]), torch.sign(mesh.normals[:, 0]))


# ---- fp64 autograd reference ---------------------------------------------------------------------------------------------------------

def _mlp_pre(w, gp, gd):
    """oracle.mlp in whatever dtype its inputs have, also returning every ReLU's / the sigma head's pre-activations."""
    W = lambda n: w[n]
    h, pres = gp, []
    for i in range(8):
        inp = torch.cat((h, gp), dim=-1) if i == 4 else h
        pre = F.linear(inp, W(f"network.point_layer.{i}.0.weight"), W(f"network.point_layer.{i}.0.bias"))
        pres.append(pre)
        h = torch.relu(pre)
    spre = F.linear(h, W("network.sigma_layer.0.weight"), W("network.sigma_layer.0.bias"))
    pres.append(spre)
    feat = F.linear(h, W("network.point_info.weight"), W("network.point_info.bias"))
    cpre = F.linear(torch.cat((gd, feat), dim=-1), W("network.dir_info.0.weight"), W("network.dir_info.0.bias"))
    pres.append(cpre)
    rgb = torch.sigmoid(F.linear(torch.relu(cpre), W("network.color_layer.0.weight"), W("network.color_layer.0.bias")))
    return rgb, torch.abs(spre).squeeze(-1), pres


def _reference(oracle, w, pts, dirs, u, v):
    """fp64 gradient of sum(sigma) and VJP of (u, v) with respect to the points: weights cast to fp64, phase fp32(x * f) cast to fp64 and
    differentiated straight through as f * (cos, -sin).  Also the per-point kink masks (sigma only, with colour): a pre-activation
    |pre| <= 1e-5 * max(1, rms of its layer at that point), where fp32 and fp64 may take different ReLU / sign decisions."""
    fp, fd = oracle.frequencies()
    w64 = OrderedDict((k, t.double()) for k, t in w.items())
    x = pts.double().requires_grad_()
    ph = x[:, :, None] * fp.double()
    ph = ph + ((pts[:, :, None] * fp).double() - ph).detach()  # value fp32(x * f), derivative f
    gp = torch.stack((torch.sin(ph), torch.cos(ph)), dim=-1).flatten(start_dim=-3)
    gd = oracle.encode(dirs, fd).double()
    rgb, sig, pres = _mlp_pre(w64, gp, gd)
    with torch.no_grad():  # the same function as the oracle's
        orgb, osig = oracle.mlp(w64, gp.detach(), gd)
        assert torch.equal(orgb, rgb) and torch.equal(osig, sig)
    g_sig, = torch.autograd.grad(sig.sum(), x, retain_graph=True)
    g_vjp, = torch.autograd.grad((sig * u.double()).sum() + (rgb * v.double()).sum(), x)
    with torch.no_grad():
        near = [(p.abs() <= 1e-5 * p.pow(2).mean(dim=-1, keepdim=True).sqrt().clamp_min(1.0)).any(dim=-1) for p in pres]
    kink_sigma = torch.stack(near[:-1]).any(dim=0)  # h0..h7 and spre; the colour branch's dir_info ReLU only matters with drgb
    return g_sig, g_vjp, kink_sigma, kink_sigma | near[-1]


def _check(g, g64, kink, what):
    g = g.cpu().double()
    err = (g - g64).norm(dim=1)
    bad = err > 1e-4 * g64.norm(dim=1) + 1e-6
    excused = bad & kink
    print(f"{what}: {int(bad.sum())} of {len(g)} points outside the bar, {int(excused.sum())} excused at kinks "
          f"({int(kink.sum())} points near a kink)")
    assert not (bad & ~kink).any(), (what, err[bad & ~kink][:5], g64[bad & ~kink][:5])
    assert excused.sum() <= 0.01 * len(g)


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("M", [1, 31, 33, 4097, CHUNK + 1, 100003])
def test_against_fp64_oracle(oracle, pkg, dev, sharp, M):
    w = oracle.make_weights(23, sharp)
    m = _model(pkg, oracle, dev, w)
    gen = torch.Generator().manual_seed(1000 + M)
    pts = (torch.rand(M, 3, generator=gen) * 8.0 - 4.0).float()
    dirs = _unit_dirs(gen, M)
    u = torch.randn(M, generator=gen)
    v = torch.randn(M, 3, generator=gen)
    _, _, dp = m.query_grad(pts.to(dev))
    _, _, dv = m.query_grad(pts.to(dev), dirs.to(dev), dsigma=u.to(dev), drgb=v.to(dev))
    g_sig, g_vjp, kink_s, kink = _reference(oracle, w, pts, dirs, u, v)
    _check(dp, g_sig, kink_s, f"grad sigma M={M} sharp={sharp}")
    _check(dv, g_vjp, kink, f"VJP M={M} sharp={sharp}")


# ---- bit-identity, determinism, autograd ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [33, CHUNK + 5])
def test_bits_determinism_and_autograd(oracle, pkg, dev, M):
    w = oracle.make_weights(4, True)
    m = _model(pkg, oracle, dev, w)
    gen = torch.Generator().manual_seed(M)
    pts = (torch.rand(M, 3, generator=gen) * 8.0 - 4.0).to(dev)
    dirs = _unit_dirs(gen, M).to(dev)
    u = torch.randn(M, generator=gen).to(dev)
    v = torch.randn(M, 3, generator=gen).to(dev)
    rgb_q, sig_q = m.query(pts, dirs)
    _, sig_s = m.query(pts)
    rgb, sig, dp = m.query_grad(pts, dirs, dsigma=u, drgb=v)
    assert torch.equal(rgb, rgb_q) and torch.equal(sig, sig_q)
    rgb2, sig2, dp2 = m.query_grad(pts, dirs, dsigma=u, drgb=v)
    assert torch.equal(dp, dp2) and torch.equal(rgb2, rgb) and torch.equal(sig2, sig)
    none, sig1, g1 = m.query_grad(pts)
    assert none is None and torch.equal(sig1, sig_s)
    assert torch.equal(m.query_grad(pts)[2], g1)
    # dirs without drgb: rgb computed, the gradient is the sigma-only one
    rgb3, _, g3 = m.query_grad(pts, dirs)
    assert torch.equal(rgb3, rgb_q) and torch.equal(g3, g1)
    # a power of two scales exactly along the whole chain
    _, _, gu = m.query_grad(pts, dsigma=u)
    _, _, g2u = m.query_grad(pts, dsigma=2.0 * u)
    assert torch.equal(g2u, 2.0 * gu)
    # autograd through model.field: query's values, query_grad's gradient bit for bit
    x = pts.clone().requires_grad_()
    frgb, fsig = m.field(x, dirs)
    assert torch.equal(frgb, rgb_q) and torch.equal(fsig, sig_q)
    gx, = torch.autograd.grad((fsig, frgb), x, (u, v))
    assert torch.equal(gx, dp)
    x = pts.clone().requires_grad_()
    none, fsig = m.field(x)
    assert none is None and torch.equal(fsig, sig_s)
    gx, = torch.autograd.grad(fsig, x, u)
    assert torch.equal(gx, gu)
    x = pts.clone().requires_grad_()
    frgb, _ = m.field(x, dirs)
    gx, = torch.autograd.grad(frgb, x, v)  # sigma unused: its upstream is zero
    assert torch.equal(gx, m.query_grad(pts, dirs, dsigma=torch.zeros_like(u), drgb=v)[2])
    # the weights are constants of model.field
    x = pts.clone().requires_grad_()
    m.field(x)[1].sum().backward()
    assert all(p.grad is None for p in m.network.parameters())
    assert torch.equal(x.grad, g1)


def test_edge_cases(oracle, pkg, dev):
    m = _model(pkg, oracle, dev, oracle.make_weights(2, False))
    e = torch.empty(0, 3, device=dev)
    rgb, sig, dp = m.query_grad(e, e, dsigma=torch.empty(0, device=dev), drgb=e)
    assert rgb.shape == (0, 3) and sig.shape == (0,) and dp.shape == (0, 3)
    assert m.query_grad(e)[2].shape == (0, 3)
    pts = torch.rand(8, 3, device=dev)
    d = torch.nn.functional.normalize(torch.rand(8, 3, device=dev), dim=1).requires_grad_()
    with pytest.raises(ValueError, match="dirs must not require grad"):
        m.field(pts.requires_grad_(), d)
    with pytest.raises(ValueError, match="drgb needs dirs"):
        m.query_grad(pts.detach(), drgb=torch.zeros(8, 3, device=dev))
    # the default normals are today's output bit for bit
    lo, hi, shape = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35), (37, 20, 45)
    level = float(m.density_grid(lo, hi, shape).median())
    a = m.extract_mesh(lo, hi, shape, level)
    b = m.extract_mesh(lo, hi, shape, level, normals="grid")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    f = m.extract_mesh(lo, hi, shape, level, normals="field")
    assert torch.equal(f.verts, a.verts) and torch.equal(f.faces, a.faces)
    from nerf_tiny_amd.nerf import field_normals

    assert torch.equal(f.normals, field_normals(m.query_grad(a.verts)[2]))
    assert torch.equal(f.rgb, m.query(a.verts, -f.normals)[0])
    length = f.normals.double().norm(dim=1)
    assert ((length - 1.0).abs() <= 1e-6).double().mean() > 0.999 and ((length == 0) | ((length - 1.0).abs() <= 1e-6)).all()


def test_runner_writes_field_normals(pkg, dev, tmp_path):
    scene = pkg.data.synthetic_scene(n_pic=4, H=32, W=32, seed=1)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=6, batch_ray=256, learning=3e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1000, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1000)
    run = pkg.NeRFRunner(continue_=False, **kw)
    assert run.trainer("train") == 5
    level = float(np.median(run.density_grid(24, save=False)))
    out = run.extract_mesh(24, level, save=True, normals="field")
    files = glob.glob(rs + "*_5_mesh24.ply")
    assert len(files) == 1 and len(out.faces) > 0
    _, V, _ = _read_ply(files[0])
    assert np.array_equal(np.stack([V["nx"], V["ny"], V["nz"]], 1), out.normals)
    from nerf_tiny_amd.nerf import field_normals

    want = field_normals(run.model.query_grad(torch.from_numpy(out.verts).to(dev))[2]).cpu().numpy()
    assert np.array_equal(out.normals, want)
