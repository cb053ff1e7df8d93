"""GPU: differentiable depth and opacity maps -- nerf_hip_forward_maps_train, nerf_hip_backward_maps,
NeRFModel.forward(maps=True) under autograd and the runner's alpha-mask loss (MASK_WEIGHT).

  A. the training forward with maps: colours and status are the plain training forward's bits; the coarse maps are the fp64 sums over the
     call's own w_c / t_c; where the colours equal the inference maps call's, the maps do too;
  B. dmaps = 0: all 24 gradients are nerf_hip_backward's bits, after either training forward, in every training mode;
  C. the fine ray stage (dC = 0, random dmaps): d sigma_fine against fp64 autograd of the fine maps over the call's own saved bundle and
     permutations; the colour branch receives exactly nothing;
  D. coarse maps only (exact fp32): every gradient at the coarse-only colour bar of the oracle's autograd;
  E. full maps + colour loss (exact fp32) with the oracle's sort order and ReLU masks replayed: inside the reference's noise band;
  F. NeRFModel.forward(maps=True): the direct calls' gradients bit for bit, a colour-only loss equal to forward's, grad_bucket mode;
  G. NeRFRunner(mask_weight > 0): one step equals the hand-written one; the gathered alpha; one RCCL rank equals the plain runner.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, golden_inputs, l2_rel, load_golden
from test_gpu_backward import CASES, GTOL, NOISE_BAND, _case, _relu_mask_image

pytestmark = pytest.mark.gpu

S, TILE, BF16, SPLIT, CORR = 1 << 0, 1 << 1, 1 << 2, 1 << 4, 1 << 5
MODES = {  # name -> (flags, rays); all at the shipped (64, 128)
    "fp32": (S, 256),
    "tile": (S | TILE, 256),
    "split_train": (S | SPLIT, 256),
    "bf16_fused": (S | BF16, 256),    # nerf_hip_forward / nerf_hip_backward fuse the per-ray stages into the field launches here
    "bf16_4096": (S | BF16, 4096),
    "corrected": (S | CORR, 256),
}
COLOUR_BRANCH = ("color_layer", "dir_info", "point_info")


def _weights_dev(oracle, seed, sharp, dev):
    p = oracle.make_weights(seed, sharp)
    return p, [v.to(dev).contiguous() for v in p.values()]


def _inputs(oracle, B, dev, seed=3):
    row, col, pb, K, Ct = oracle.fern_inputs(B, seed=seed)
    return row.to(dev).contiguous(), col.to(dev).contiguous(), pb.float().to(dev).contiguous(), K, Ct


def _status(pkg, ws):
    st = ctypes.c_uint32(0)
    pkg._abi.check(pkg._abi.lib().nerf_hip_read_status(ws.data_ptr(), ws.numel(), ctypes.byref(st), None))
    return int(st.value)


def _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, kind):
    """kind: "plain" (nerf_hip_forward), "train_maps" (nerf_hip_forward_maps_train), "infer_maps" (nerf_hip_forward_maps, flags without
    SAVE_FOR_BACKWARD) on a fresh workspace -> (C_c, C_f, maps or None, status, ws)."""
    _abi = pkg._abi
    dev = P[0].device
    B = row.shape[0]
    n = _abi.ws_bytes(B, Nc, Nf, flags)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    Cc = torch.full((B, 3), float("nan"), device=dev)
    Cf = torch.full((B, 3), float("nan"), device=dev)
    K9 = _abi.f32_array(K.reshape(-1).tolist())
    args = (_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, None, B, Nc, Nf, pkg.nerf.LAST_DELTA, Cc.data_ptr(), Cf.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    M = None
    if kind == "plain":
        _abi.check(_abi.lib().nerf_hip_forward(*args, ws.data_ptr(), n, flags, stream))
    else:
        M = torch.full((B, 4), float("nan"), device=dev)
        fn = _abi.lib().nerf_hip_forward_maps_train if kind == "train_maps" else _abi.lib().nerf_hip_forward_maps
        _abi.check(fn(*args, M.data_ptr(), ws.data_ptr(), n, flags, stream))
    torch.cuda.synchronize()
    return Cc, Cf, M, _status(pkg, ws), ws


def _bwd(pkg, P, ws, B, Nc, Nf, flags, dCc, dCf, dmaps=None):
    """nerf_hip_backward (dmaps None) / nerf_hip_backward_maps on the workspace of a training forward -> 24 gradient tensors."""
    _abi = pkg._abi
    G = [torch.full_like(p, float("nan")) for p in P]
    stream = torch.cuda.current_stream(P[0].device).cuda_stream
    if dmaps is None:
        _abi.check(_abi.lib().nerf_hip_backward(_abi.ptr_array(P), dCc.data_ptr(), dCf.data_ptr(), None, B, Nc, Nf, pkg.nerf.LAST_DELTA,
                                                _abi.ptr_array(G), ws.data_ptr(), ws.numel(), flags, stream))
    else:
        _abi.check(_abi.lib().nerf_hip_backward_maps(_abi.ptr_array(P), dCc.data_ptr(), dCf.data_ptr(), dmaps.data_ptr(), None, B, Nc, Nf,
                                                     pkg.nerf.LAST_DELTA, _abi.ptr_array(G), ws.data_ptr(), ws.numel(), flags, stream, None))
    torch.cuda.synchronize()
    return G


def _names(oracle):
    return list(oracle.make_weights(0, False).keys())


# ---------------------------------------------------------------------------------------------------------------
# A. the training forward with maps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_training_forward_with_maps(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev)
    c0, f0, _, s0, _ = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "plain")
    c1, f1, M, s1, ws = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")
    assert torch.equal(c0, c1) and torch.equal(f0, f1), mode
    assert s0 == s1
    assert torch.isfinite(M).all()
    w_c = pkg._abi.ws_view(ws, B, Nc, Nf, flags, "w_c", (B, Nc)).double().cpu()
    t_c = pkg._abi.ws_view(ws, B, Nc, Nf, flags, "t_c", (B, Nc)).double().cpu()
    Md = M.double().cpu()
    D, A = (w_c * t_c).sum(1), w_c.sum(1)
    assert float(((Md[:, 0] - D).abs() / D.abs().clamp_min(1e-20)).max()) <= 1e-6
    assert float((Md[:, 1] - A).abs().max()) <= 1e-6
    # the inference maps call of the same mode: where its colours are the training call's bits, so are its maps
    c2, f2, M2, _, _ = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags & ~S, "infer_maps")
    same = (c2 == c1).all(1) & (f2 == f1).all(1)
    if mode in ("fp32", "tile", "corrected"):
        # the exact fp32 forward is one kernel family for training and inference: every ray's colours, and so its maps, are the same bits
        assert bool(same.all()), mode
        assert torch.equal(M2, M)
    else:
        # split-fp32 and bf16 inference run other kernels than their training forwards (field_fwd_split / field_fwd_bf16x): equal colour bits
        # of a ray do not imply equal samples -- a sample whose weight is below the colour sums' last bit still moves D / A
        d = float((M2[same] - M[same]).abs().max()) if bool(same.any()) else 0.0
        print(f"{mode}: {int(same.sum())} / {B} rays with the inference call's colour bits; their maps differ by <= {d:.2e}")
        assert d <= 1e-2


# ---------------------------------------------------------------------------------------------------------------
# B. zero upstream of the maps: nerf_hip_backward's bits
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forward", ["plain", "train_maps"])
@pytest.mark.parametrize("mode", list(MODES))
def test_zero_dmaps_gives_the_plain_backward(oracle, pkg, dev, mode, forward):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev)
    gen = torch.Generator().manual_seed(11)
    dCc, dCf = (torch.randn(B, 3, generator=gen).to(dev) for _ in range(2))
    ref = _bwd(pkg, P, _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, forward)[4], B, Nc, Nf, flags, dCc, dCf)
    got = _bwd(pkg, P, _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, forward)[4], B, Nc, Nf, flags, dCc, dCf, torch.zeros(B, 4, device=dev))
    for k, a, b in zip(_names(oracle), got, ref):
        assert torch.equal(a, b), (mode, forward, k, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# C. the fine ray stage against fp64 autograd over the call's own saves
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_fine_ray_stage_against_fp64(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    N = Nc + Nf
    _, P = _weights_dev(oracle, 1, False, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev, seed=5)
    _, _, _, _, ws = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")
    view = lambda name, shape, dt=None: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, shape, dt)
    bundle = view("bundle", (B, N, 5)).double().cpu()
    perm = view("perm", (B, 5, N), torch.int16).long().cpu()
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(B, 4, generator=gen)
    zero = torch.zeros(B, 3, device=dev)
    G = _bwd(pkg, P, ws, B, Nc, Nf, flags, zero, zero, g.to(dev))
    # fp64: D_f = sum_k w_k t_s,k, A_f = sum_k w_k over the sorted channels; d / d sigma_sorted un-sorted through the sigma channel's permutation
    t_s = bundle[:, :, 0]
    sig = bundle[:, :, 4].clone().requires_grad_(True)
    delta = torch.cat((t_s[:, 1:] - t_s[:, :-1], torch.full((B, 1), pkg.nerf.LAST_DELTA, dtype=torch.float64)), 1)
    w = oracle.weights_from_sigma(delta, sig)
    ((w * t_s).sum(1) * g[:, 2].double() + w.sum(1) * g[:, 3].double()).sum().backward()
    dsig = torch.zeros(B, N, dtype=torch.float64).scatter_(1, perm[:, 4], sig.grad)
    got = view("dsig_f", (B, Nf)).double().cpu()
    e = l2_rel(got, dsig[:, Nc:])
    print(f"{mode}: d sigma_fine L2-rel {e:.2e}")
    assert e < 3e-4, (mode, e)
    assert bool((view("drgb_c", (B, Nc, 3)) == 0).all()) and bool((view("drgb_f", (B, Nf, 3)) == 0).all())
    for k, q in zip(_names(oracle), G):
        assert torch.isfinite(q).all(), k
        if any(s in k for s in COLOUR_BRANCH):
            assert bool((q == 0).all()), (mode, k)


# ---------------------------------------------------------------------------------------------------------------
# D. coarse maps only, E. full maps + colour loss with the reference's decisions replayed (exact fp32)
# ---------------------------------------------------------------------------------------------------------------
def _oracle_maps_grads(oracle, w, inputs, Nc, Nf, g, colour):
    row, col, pb, K, Ct = inputs
    p = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    st = {}
    Cc, Cf = oracle.render(p, row, col, pb, K, Nc, Nf, stages=st)
    maps = torch.stack(((st["w_c"] * st["t_c"]).sum(1), st["w_c"].sum(1), (st["w"] * st["t_s"]).sum(1), st["w"].sum(1)), 1)
    loss = (maps * g).sum()
    if colour:
        loss = loss + oracle.ray_loss(Cc, Cf, Ct)
    loss.backward()
    return p, st


def _shift(oracle, w, inputs, Nc, Nf, g, colour, p):
    """Per tensor: how far the oracle's OWN gradient of this loss moves under a seeded 1e-6 relative weight perturbation (as
    tests/test_gpu_backward.py::_sensitivity_band).  The depth maps weight every sample by its depth, which makes layer 0's gradient
    ill-conditioned where the colour loss's is not: a bar below twice this shift would ask for more than fp32 holds."""
    gen = torch.Generator().manual_seed(1)
    wp = {k: v * (1.0 + 1e-6 * torch.randn(v.shape, generator=gen)) for k, v in w.items()}
    p1, _ = _oracle_maps_grads(oracle, wp, inputs, Nc, Nf, g, colour)
    return {k: l2_rel(p1[k].grad, p[k].grad) for k in p}


def _model(pkg, w, B, Nc, Nf, dev):
    m = pkg.NeRFModel(Nc, Nf, B)
    m.load_state_dict(w)
    return m.to(dev)


@pytest.mark.parametrize("name", CASES)
def test_coarse_maps_gradient_against_the_oracle(oracle, pkg, dev, name):
    g_, inputs, Nc, Nf, w = _case(oracle, name, max_rays=256)
    row, col, pb, K, Ct = inputs
    B = row.shape[0]
    gen = torch.Generator().manual_seed(2)
    g = torch.randn(B, 4, generator=gen)
    g[:, 2:] = 0
    p, _ = _oracle_maps_grads(oracle, w, inputs, Nc, Nf, g, colour=False)
    m = _model(pkg, w, B, Nc, Nf, dev)
    _, _, M = m(row, col, pb, K, maps=True)
    (M * g.to(dev)).sum().backward()
    shift = _shift(oracle, w, inputs, Nc, Nf, g, False, p)
    worst = 0.0
    for (k, ref), q in zip(p.items(), m.network.parameters()):
        if any(s in k for s in COLOUR_BRANCH):
            assert bool((q.grad == 0).all()), k
            continue
        e = l2_rel(q.grad, ref.grad)
        worst = max(worst, e)
        assert e < max(GTOL, 2 * shift[k]), (k, e, shift[k])
    print(f"{name}: coarse maps, worst grad L2-rel {worst:.2e}")


@pytest.mark.parametrize("name", CASES)
def test_full_maps_and_colour_gradient_given_reference_decisions(oracle, pkg, dev, name):
    g_, inputs, Nc, Nf, w = _case(oracle, name)
    row, col, pb, K, Ct = inputs
    B, N = row.shape[0], Nc + Nf
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(B, 4, generator=gen)
    p, st = _oracle_maps_grads(oracle, w, inputs, Nc, Nf, g, colour=True)
    st = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in st.items()}
    m = _model(pkg, w, B, Nc, Nf, dev)
    Cc, Cf, M = m(row, col, pb, K, maps=True)
    # replay the oracle's sort order and ReLU masks into the workspace (as tests/test_gpu_backward.py::_train_step)
    view = lambda nm, shape, dt=None: pkg._abi.ws_view(m.last_workspace, B, Nc, Nf, S, nm, shape, dt)
    vals = torch.cat((torch.cat((view("t_c", (B, Nc)), view("t_f", (B, Nf))), 1).unsqueeze(2),
                      torch.cat((view("rgb_c", (B, Nc, 3)), view("rgb_f", (B, Nf, 3))), 1),
                      torch.cat((view("sig_c", (B, Nc)), view("sig_f", (B, Nf))), 1).unsqueeze(2)), dim=2)
    perm = st["perm"].to(dev)
    view("bundle", (B, N, 5)).copy_(torch.gather(vals, 1, perm))
    view("perm", (B, 5, N), torch.int16).copy_(perm.permute(0, 2, 1).to(torch.int16))
    f_p, _ = oracle.frequencies()
    imgs = []
    for pts, n in ((st["pts_c"], Nc), (st["pts_f"], Nf)):
        with torch.no_grad():
            _, _, hidden, _, _ = oracle.mlp(w, oracle.encode(pts, f_p), st["gd"][:, None, :].expand(-1, n, -1), return_hidden=True)
        imgs.append(_relu_mask_image([h.reshape(-1, 256) for h in hidden], (B * n + 63) // 64))
    img = torch.cat(imgs, dim=1)
    view("masks", tuple(img.shape), torch.int16).copy_(img.to(dev))
    (m.ray_loss(Cc, Cf, Ct.to(dev)) + (M * g.to(dev)).sum()).backward()
    shift = None
    worst = 0.0
    for (k, ref), q in zip(p.items(), m.network.parameters()):
        e = l2_rel(q.grad, ref.grad)
        worst = max(worst, e)
        if e >= NOISE_BAND:  # (only then: the band costs another oracle run)
            shift = shift or _shift(oracle, w, inputs, Nc, Nf, g, True, p)
            assert e < 2 * shift[k], (k, e, shift[k])
    print(f"{name}: maps + colour loss, worst grad L2-rel (reference decisions replayed) {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------
# F. NeRFModel.forward(maps=True)
# ---------------------------------------------------------------------------------------------------------------
def _set_mode(m, flags):
    m.force_tile_kernel = bool(flags & TILE)
    m.bf16_mlp = bool(flags & BF16)
    m.split_train = bool(flags & SPLIT)
    m.corrected = bool(flags & CORR)


@pytest.mark.parametrize("mode", list(MODES))
def test_model_forward_maps_under_autograd(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    w, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, Ct = _inputs(oracle, B, dev)
    m = _model(pkg, w, B, Nc, Nf, dev)
    _set_mode(m, flags)
    gen = torch.Generator().manual_seed(5)
    a, b, g = torch.randn(B, 3, generator=gen).to(dev), torch.randn(B, 3, generator=gen).to(dev), torch.randn(B, 4, generator=gen).to(dev)
    Cc, Cf, M = m(row, col, pb, K, maps=True)
    assert Cc.requires_grad and M.requires_grad
    ((Cc * a).sum() + (Cf * b).sum() + (M * g).sum()).backward()
    got = [q.grad.clone() for q in m.network.parameters()]
    c1, f1, M1, _, ws = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")
    assert torch.equal(Cc, c1) and torch.equal(Cf, f1) and torch.equal(M, M1)
    ref = _bwd(pkg, P, ws, B, Nc, Nf, flags, a, b, g)
    for k, x, y in zip(_names(oracle), got, ref):
        assert torch.equal(x, y), (mode, k)
    # a colour-only loss through maps=True: forward's gradients (an upstream autograd hands over as None counts as zero)
    m.zero_grad(set_to_none=True)
    Cc, Cf, M = m(row, col, pb, K, maps=True)
    m.ray_loss(Cc, Cf, Ct.to(dev)).backward()
    got = [q.grad.clone() for q in m.network.parameters()]
    m.zero_grad(set_to_none=True)
    Cc0, Cf0 = m(row, col, pb, K)
    m.ray_loss(Cc0, Cf0, Ct.to(dev)).backward()
    assert torch.equal(Cc, Cc0) and torch.equal(Cf, Cf0)
    for (k, q), x in zip(m.network.named_parameters(), got):
        assert torch.equal(x, q.grad), (mode, k)
    # the maps alone (the colours' upstream None)
    m.zero_grad(set_to_none=True)
    _, _, M = m(row, col, pb, K, maps=True)
    (M * g).sum().backward()
    ref = _bwd(pkg, P, _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")[4], B, Nc, Nf, flags, torch.zeros_like(a), torch.zeros_like(b), g)
    for (k, q), y in zip(m.network.named_parameters(), ref):
        assert torch.equal(q.grad, y), (mode, k)


def test_model_forward_maps_without_grad_is_the_inference_call(oracle, pkg, dev):
    w, P = _weights_dev(oracle, 4, True, dev)
    B = 256
    row, col, pb, K, _ = _inputs(oracle, B, dev)
    m = _model(pkg, w, B, 64, 128, dev)
    with torch.no_grad():
        Cc, Cf, M = m(row, col, pb, K, maps=True)
    assert not M.requires_grad
    c1, f1, M1, _, _ = _fwd(pkg, P, row, col, pb, K, 64, 128, 0, "infer_maps")
    assert torch.equal(Cc, c1) and torch.equal(Cf, f1) and torch.equal(M, M1)


def test_model_forward_maps_bucket_and_generation_guard(oracle, pkg, dev):
    from nerf_tiny_amd import parallel as par

    w, _ = _weights_dev(oracle, 4, True, dev)
    B = 256
    row, col, pb, K, Ct = _inputs(oracle, B, dev)
    m = _model(pkg, w, B, 64, 128, dev)
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(B, 4, generator=gen).to(dev)
    loss = lambda out: m.ray_loss(out[0], out[1], Ct.to(dev)) + (out[2] * g).sum()
    loss(m(row, col, pb, K, maps=True)).backward()
    ref = [q.grad.clone() for q in m.network.parameters()]
    bucket = par.GradBucket(m.network.parameters())
    m.grad_bucket = bucket
    try:
        loss(m(row, col, pb, K, maps=True)).backward()
        assert bucket.pending
        for q, v, r in zip(m.network.parameters(), bucket.views, ref):
            assert q.grad.data_ptr() == v.data_ptr() and torch.equal(v, r)
        with pytest.raises(RuntimeError, match="second backward"):
            loss(m(row, col, pb, K, maps=True)).backward()
        bucket.consume()
    finally:
        m.grad_bucket = None
    first = loss(m(row, col, pb, K, maps=True))
    loss(m(row, col, pb, K, maps=True))  # a later training forward on the same workspace
    with pytest.raises(RuntimeError, match="reused by a later training forward"):
        first.backward()


# ---------------------------------------------------------------------------------------------------------------
# G. the runner's alpha-mask loss
# ---------------------------------------------------------------------------------------------------------------
def _runner(pkg, tmp, scene, mask_weight, iters=1):
    return pkg.NeRFRunner(gpu=0, img_dir="", results_path=str(tmp / "res") + "/", ckpt_path=str(tmp / "ck") + "/", low_res=1, total_iter=iters,
                          batch_ray=256, learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=100,
                          decay_end=10000, sched="EXP", datasets={"train": scene, "val": scene, "test": scene}, log_every=1,
                          on_resample_fault="ignore", distributed=False, mask_weight=mask_weight)


def test_device_rays_yield_alpha_only_when_asked(pkg, dev):
    scene = pkg.data.analytic_sphere_scene(n_pic=2, H=16, W=16, device=str(dev))
    a = scene.all_alpha
    assert a.shape == (2 * 16 * 16,) and set(a.unique().tolist()) == {0.0, 1.0}
    # alpha 1 exactly where the image is not the white background (the sphere's shading never reaches (1, 1, 1))
    assert torch.equal(a == 0, (scene.all_pix == 1).all(1))
    rays = pkg.data.DeviceRays(scene, dev, seed=1)
    idx = torch.randperm(len(rays), device=dev)[:100]
    plain = rays.gather(idx)
    full = rays.gather(idx, with_alpha=True)
    assert len(plain) == 5 and len(full) == 6
    for x, y in zip(plain, full):
        assert torch.equal(x, y)
    assert torch.equal(full[5], a.to(dev)[idx])
    assert len(next(rays.epoch(64))) == 5 and len(next(rays.epoch(64, with_alpha=True))) == 6
    sh = next(rays.epoch_sharded(64, 0, 1))
    sha = next(rays.epoch_sharded(64, 0, 1, with_alpha=True))
    assert len(sh) == 6 and len(sha) == 7 and isinstance(sha[6], tuple) and sha[5].shape == (64,)
    with pytest.raises(ValueError, match="alpha"):
        pkg.data.DeviceRays(pkg.data.synthetic_scene(n_pic=2, H=8, W=8), dev).gather(idx[:4] % 128, with_alpha=True)


def test_runner_mask_step_equals_the_hand_written_step(pkg, dev, tmp_path):
    scene = pkg.data.analytic_sphere_scene(n_pic=3, H=24, W=24, device=str(dev))
    lam = 0.5
    torch.manual_seed(0)
    run = _runner(pkg, tmp_path / "a", scene, lam)
    losses = []
    run.writer.add_scalar = lambda tag, v, it: losses.append((tag, float(v)))
    assert run.trainer("train") == 0
    torch.manual_seed(0)
    hand = _runner(pkg, tmp_path / "b", scene, lam)
    m = hand.model
    row, col, pix, pb, pic, alpha = next(hand.train_rays.epoch(hand.batch_ray, with_alpha=True))
    Cc, Cf, M = m(row, col, pb, hand.K_inv, maps=True)
    loss = m.ray_loss(Cc, Cf, pix) + lam * m.mask_loss(M, alpha)
    loss.backward()
    hand.optimizer.step()
    for (k, a), b in zip(run.model.network.named_parameters(), m.network.parameters()):
        assert torch.equal(a, b), k
    assert [v for t, v in losses if t.startswith("loss/")] == [float(loss)]
    # the mask term is what it says: sum of both opacity maps' squared errors against alpha
    with torch.no_grad():
        want = ((M[:, 1] - alpha) ** 2).sum() + ((M[:, 3] - alpha) ** 2).sum()
    assert float((m.mask_loss(M, alpha) - want).abs()) <= 1e-6 * max(1.0, float(want))


def test_runner_refuses_a_dataset_without_alpha(pkg, dev, tmp_path):
    with pytest.raises(ValueError, match="alpha"):
        _runner(pkg, tmp_path, pkg.data.synthetic_scene(n_pic=2, H=8, W=8), 0.1)


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def _run_ranks(n, out, extra=(), timeout=500):
    import socket

    tool = os.path.join(ROOT, "tests", "tools", "mask_runner_rank.py")
    if n == 0:
        cmd = [sys.executable, tool, out, *extra]
    else:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), tool, out, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=_env(), timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "MASK-RUNNER-OK" in r.stdout
    return torch.load(os.path.join(out, "result.pt"), weights_only=False)


@pytest.mark.timeout(900)
def test_mask_runner_single_rank_rccl_equals_plain_runner(tmp_path):
    plain = _run_ranks(0, str(tmp_path / "plain"))
    dp = _run_ranks(1, str(tmp_path / "dp1"), ("--force-dist",))
    assert plain["distributed"] is False and dp["distributed"] is True and dp["ranks"] == 1
    assert len(dp["losses"]) == 6
    assert plain["losses"] == dp["losses"]
    assert torch.equal(plain["weights"], dp["weights"])
    assert torch.equal(plain["frame"], dp["frame"])
