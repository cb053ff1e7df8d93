"""GPU: the lazy ReLU of the inference forward goes through LDS (ds_write_b128 from the accumulators, ds_max_i32 with 0, ds_read_b128;
csrc/field_fwd_reg.hip) while the saving forward keeps fmaxf on the VALU.  Both must give the same bits for every non-NaN
pre-activation.  tests/test_gpu_layers.py::test_inference_and_saving_forward_give_the_same_bits holds that on ordinary weights; here the
weights put the values an integer maximum could get wrong into every layer, and the point-query, density-grid and gradient-query forms
(the other instantiations of the same kernel) are held to the ray path on those weights.

The special units: a zero weight row whose bias is the value, so the unit's pre-activation is that value for every sample (a -0 bias
becomes +0 in the accumulator: -0 * 1 + 0).  The column that reads the unit in the next layer is scaled by 2^-e (value = m * 2^e) so that
a wrong activation -- a negative let through, a subnormal flushed, a huge value clipped -- moves the next layer by about 0.5 instead
of vanishing or overflowing; nothing becomes infinite, so no NaN arises (integer max and fmaxf differ on NaN, and only there)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = 3.4028234663852886e38
SPECIAL = [0.0, -0.0, 2.0 ** -130, -(2.0 ** -130), 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126),
           2.0 ** 100, -(2.0 ** 100), FLT_MAX, -FLT_MAX]


def _units(l, n):
    return [(13 + 29 * l + 17 * i) % n for i in range(len(SPECIAL))]


def _col_scale(v, sign):
    if v == 0.0:
        return None
    e = math.frexp(abs(v))[1]  # |v| = m * 2^e, m in [0.5, 1)
    return sign * math.ldexp(1.0, max(min(-e, 126), -126))  # |v| * scale = m (FLT_MAX: 2^-126 * 2^128 m = 4 m)


def special_weights(oracle, seed):
    w = {k: v.clone() for k, v in oracle.make_weights(seed, sharp=True).items()}
    for l in range(8):
        readers = ([(f"network.point_layer.{l + 1}.0.weight", None)] if l < 7 else
                   [("network.sigma_layer.0.weight", None), ("network.point_info.weight", None)])
        for i, (u, v) in enumerate(zip(_units(l, 256), SPECIAL)):
            w[f"network.point_layer.{l}.0.weight"][u] = 0
            w[f"network.point_layer.{l}.0.bias"][u] = v
            s = _col_scale(v, -1.0 if i % 4 < 2 else 1.0)
            if s is not None:
                for name, _ in readers:
                    # one reader row per unit keeps the next pre-activations O(1) whatever the value's mantissa
                    col = torch.zeros_like(w[name][:, u])
                    col[(u + 5) % col.shape[0]] = s
                    w[name][:, u] = col
    for i, (u, v) in enumerate(zip(_units(3, 128), SPECIAL)):  # dir_info: feature and direction columns both zero
        w["network.dir_info.0.weight"][u] = 0
        w["network.dir_info.0.bias"][u] = v
        s = _col_scale(v, 1.0 if i % 4 < 2 else -1.0)
        if s is not None:
            col = torch.zeros(3)
            col[i % 3] = s
            w["network.color_layer.0.weight"][:, u] = col
    return w


def _model(pkg, w, B, Nc, Nf, dev):
    m = pkg.NeRFModel(Nc, Nf, B)
    m.load_state_dict(w)
    return m.to(dev)


def _inputs(oracle, B, Nc, Nf):
    return oracle.lego_inputs(B, seed=5) if (Nc, Nf) == (64, 128) else oracle.fern_inputs(B, seed=9)


def test_special_values_reach_the_device_as_written(oracle, pkg, dev):
    """the premise: the biases arrive bit for bit (subnormals and -0 included) and the special rows are zero."""
    w = special_weights(oracle, 8)
    m = _model(pkg, w, 8, 64, 128, dev)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for l in range(8):
        b = sd[f"network.point_layer.{l}.0.bias"][_units(l, 256)]
        assert torch.equal(b.view(torch.int32), torch.tensor(SPECIAL, dtype=torch.float32).view(torch.int32))
        assert float(sd[f"network.point_layer.{l}.0.weight"][_units(l, 256)].abs().max()) == 0.0


@pytest.mark.parametrize("B,Nc,Nf", [(4096, 64, 128), (130, 31, 65)])
def test_special_preactivations_inference_equals_saving_forward(oracle, pkg, dev, B, Nc, Nf):
    from nerf_tiny_amd import _abi

    row, col, pb, K, _ = _inputs(oracle, B, Nc, Nf)
    m = _model(pkg, special_weights(oracle, 8), B, Nc, Nf, dev)
    names = [("sig_c", (B * Nc,)), ("rgb_c", (B * Nc, 3)), ("t_f", (B * Nf,)), ("sig_f", (B * Nf,)), ("rgb_f", (B * Nf, 3))]
    with torch.no_grad():
        Ci = [c.clone() for c in m(row, col, pb, K)]
    ws = m._ws[0][1]
    inf = [_abi.ws_view(ws, B, Nc, Nf, 0, n, s).clone() for n, s in names]
    Ct = m(row, col, pb, K)
    ws = m.last_workspace
    tr = [_abi.ws_view(ws, B, Nc, Nf, _abi.SAVE_FOR_BACKWARD, n, s) for n, s in names]
    for (n, _), a, b in zip(names, inf, tr):
        assert bool(torch.isfinite(a).all()), n  # (the construction keeps everything finite: equality below is not NaN-blind)
        assert torch.equal(a, b), n
    assert torch.equal(Ci[0], Ct[0].detach()) and torch.equal(Ci[1], Ct[1].detach())
    # the special units matter: without them the field is a different one (a ReLU that dropped them all would not pass unseen)
    plain = _model(pkg, oracle.make_weights(8, sharp=True), B, Nc, Nf, dev)
    with torch.no_grad():
        Cp = plain(row, col, pb, K)
    assert not torch.equal(Cp[1], Ci[1])


@pytest.mark.parametrize("B,N", [(256, 64), (37, 31)])
def test_point_query_and_grid_match_the_ray_path_on_special_weights(oracle, pkg, dev, B, N):
    row, col, pb, K, _ = _inputs(oracle, B, N, 128 if N == 64 else 65)
    m = _model(pkg, special_weights(oracle, 3), 8, 64, 128, dev)
    pd = [p.detach() for p in m.network.parameters()]
    R, o, near, far = oracle.poses_extract(pb)
    t = oracle.coarse_depths(near, far, N)
    rgb_f, sig_f = pkg.ops.field(pd, row.to(dev), col.to(dev), pb.float().to(dev), K, t.to(dev))
    pts = oracle.sample_points(R, o, oracle.camera_dirs(row, col, K), t).reshape(-1, 3)
    _, d_wrd, _ = pkg.ops.rays(row.to(dev), col.to(dev), pb.float().to(dev), K, N)
    dirs = d_wrd[:, None, :].expand(B, N, 3).reshape(-1, 3)
    rgb_q, sig_q = m.query(pts.to(dev), dirs)
    assert bool(torch.isfinite(rgb_f).all()) and bool(torch.isfinite(sig_f).all())
    assert torch.equal(rgb_q, rgb_f.reshape(-1, 3))
    assert torch.equal(sig_q, sig_f.reshape(-1))
    _, sig_s = m.query(pts.to(dev))
    assert torch.equal(sig_s, sig_f.reshape(-1))
    # the lattice form: the same points formed in the kernel
    shape = (9, 7, 11)
    lo, hi = (-1.3, -0.45, -2.1), (1.1, 0.8, 0.35)
    grid = m.density_grid(lo, hi, shape)
    lo32 = torch.tensor(lo, dtype=torch.float32)
    step = (torch.tensor(hi, dtype=torch.float32) - lo32) / torch.tensor([n - 1 for n in shape], dtype=torch.float32)
    axes = [lo32[c] + torch.arange(shape[c], dtype=torch.float32) * step[c] for c in range(3)]
    lat = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    _, sig_l = m.query(lat.to(dev))
    assert torch.equal(grid.reshape(-1), sig_l)


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("M", [1, 33, 4097])
def test_gradient_query_forward_gives_the_query_bits(oracle, pkg, dev, special, M):
    """query_grad's forward is the same kernel with the mask-only save: its sigma / rgb are query()'s, with and without colour."""
    w = special_weights(oracle, 11) if special else oracle.make_weights(11, sharp=True)
    m = _model(pkg, w, 8, 64, 128, dev)
    gen = torch.Generator().manual_seed(M)
    pts = (torch.rand(M, 3, generator=gen) * 8.0 - 4.0).float().to(dev)
    d = torch.randn(M, 3, generator=gen)
    dirs = (d / d.norm(dim=1, keepdim=True)).to(dev)
    rgb_q, sig_q = m.query(pts, dirs)
    rgb_g, sig_g, dp = m.query_grad(pts, dirs, drgb=torch.ones(M, 3, device=dev))
    assert torch.equal(rgb_g, rgb_q) and torch.equal(sig_g, sig_q)
    assert dp.shape == (M, 3)
    _, sig_s = m.query(pts)
    _, sig_gs, _ = m.query_grad(pts)
    assert torch.equal(sig_gs, sig_s) and torch.equal(sig_s, sig_q)
