"""GPU: the distortion loss on the device (rule DL of include/nerf_hip.h) -- the distortion forms of k_coarse_x / k_merge_x,
k_coarse_bwd_x / k_merge_bwd_x through their stage entries, nerf_hip_forward_distortion_train / nerf_hip_backward_distortion,
NeRFModel.forward(maps=True, distortion=True) under autograd and the runner's DIST_WEIGHT.

  A. stage forward, at every size of tests/ray_stage_reference.py, joint 0 and 1, and on exact ties: the outputs shared with the maps / train
     entries are their bits; L_c, L_f against the float64 rule over the device's OWN w_c / t_c and its own sorted bundle and w.
     The bar is derived, not measured: the kernel forms L in float64 and rounds it once to fp32.  For t <= 8, W <= 1, r <= 1/3, N <= 2048 the
     float64 result's absolute error is below N 2^-53 t W^2 r (a small constant) < 1e-11, and the one rounding costs at most 2^-24 |L|: so
     |L - L_ref| <= 2^-22 |L_ref| + 1e-10.  A miss means fp32 crept into the accumulation.
  B. stage backward, same sizes and ties, random ddist, with and without dC / dmaps: all five merge gradients and both coarse gradients against
     the float64 graph, at the bars of tests/test_gpu_ray_stages.py -- max(2.5 (e32 + e_exp), 1e-6), the fp32 CPU graph and the exp-bias graph
     both with the distortion term --; every element written; the coarse call ADDS; ddist = 0 gives the maps backward's values; the waves
     behind the batch store nothing.
  C. whole call, every mode of test_gpu_maps_train.MODES at (64, 128): colours, maps, status and the bundle / perm saves are
     nerf_hip_forward_maps_train's bits; dist at bar A against the call's own saves; ddist = 0 equals nerf_hip_backward_maps on all 24 tensors;
     with dC = 0, dmaps = 0 and random ddist, d sigma_fine against float64 autograd over the call's own saves (< 3e-4 L2-rel, the bar of that
     file's test C: the term enters the same fp32 chain at the same point) and the colour branch exactly zero; the workspace is the maps call's.
  D. Python: forward(maps=True, distortion=True) under autograd gives the direct calls' gradients bit for bit; a colour-only loss through it
     equals forward's; grad_bucket mode; both ValueErrors; one NeRFRunner(dist_weight > 0) step equals the hand-written
     regularized_train_step; one single-rank RCCL step equals the plain runner; dist_weight = 0 leaves a runner step the one-call train_step's.
"""
import os
import subprocess
import sys

import pytest
import torch

import distortion_reference as DR
import ray_stage_reference as R
from conftest import ROOT, l2_rel
from test_gpu_maps_train import COLOUR_BRANCH, MODES, _bwd, _env, _fwd, _inputs, _model, _names, _set_mode, _status, _weights_dev
from test_gpu_ray_stages import NAMES_D, Bars, _bits, _case, _exp_low, _merge_s32, _same_values, _tie_case

pytestmark = pytest.mark.gpu

SIZES = list(R.CASES)
F32, F64 = torch.float32, torch.float64
S = 1


def _assert_bar_a(label, got, ref):
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref).abs()
    bar = 2.0 ** -22 * ref.abs() + 1e-10
    i = int((err / bar).argmax())
    print(f"{label}: worst |L - L_ref| = {float(err[i]):.3e} at L_ref = {float(ref[i]):.6e} (bar {float(bar[i]):.3e}, {float(err[i] / bar[i]):.3f} of it)")
    assert bool(torch.isfinite(got).all()) and bool((err <= bar).all()), (label, float(err[i]), float(bar[i]))


def _ddist(B, seed=21):
    return torch.randn(B, 2, generator=torch.Generator().manual_seed(seed))


def _tie_near_far(B):
    return torch.full((B,), 1.5), torch.full((B,), 6.5)  # (the tied depths lie in [2, 6.01])


# ---------------------------------------------------------------------------------------------------------------
# A. stage forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_coarse_stage_forward(pkg, dev, Nc, Nf):
    c = _case(pkg, dev, Nc, Nf)
    o, d = c["o"], c["d"]
    w_c, C_c, t_f, status, maps = c["coarse"]
    got = pkg.ops.coarse_composite_distortion(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], Nf)
    for a, b in zip(got[:3], (w_c, C_c, t_f)):
        assert torch.equal(_bits(a), _bits(b))
    assert got[3] == status and _same_values(got[4], maps) and bool(torch.isnan(got[4][:, 2:]).all())
    dist = got[5]
    assert bool(torch.isnan(dist[:, 1]).all())  # the fine column is not this kernel's
    _assert_bar_a(f"A coarse ({Nc}, {Nf})", dist[:, 0], DR.distortion(o["t_c"].double(), w_c.double().cpu(), o["near"].double(), o["far"].double()))
    # a call of 5 rays (two workgroups, three waves behind the batch): the same bits for its rays, nothing stored behind them
    part = pkg.ops.coarse_composite_distortion(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], Nf, sentinel=123.0, rays=5)[5]
    assert torch.equal(_bits(part[:5, 0]), _bits(dist[:5, 0])) and float(part[5, 0]) == 123.0 and bool((part[:, 1] == 123.0).all())


def _merge_forward(pkg, label, chans, near, far, ref_out, joint):
    got = pkg.ops.merge_composite_distortion(*chans, near, far, last=R.LAST, joint=bool(joint))
    for a, b in zip(got[:4], ref_out[:4]):
        assert torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert _same_values(got[4], ref_out[4]) and bool(torch.isnan(got[4][:, :2]).all())
    dist = got[5]
    assert bool(torch.isnan(dist[:, 0]).all())  # the coarse column is not this kernel's
    _assert_bar_a(label, dist[:, 1], DR.distortion(got[0][:, :, 0].double().cpu(), got[1].double().cpu(), near.double(), far.double()))


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_merge_stage_forward(pkg, dev, Nc, Nf, joint):
    c = _case(pkg, dev, Nc, Nf)
    o, d = c["o"], c["d"]
    chans = (d["t_c"], c["coarse"][2], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"])
    _merge_forward(pkg, f"A merge ({Nc}, {Nf}) joint={joint}", chans, o["near"], o["far"], c["merge", joint], joint)


@pytest.mark.parametrize("joint", [0, 1])
def test_merge_stage_forward_on_exact_ties(pkg, dev, joint):
    t = _tie_case(pkg, dev)
    d = t["d"]
    near, far = _tie_near_far(R.B_RAYS)
    chans = (d["t_c"], d["t_f"], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"])
    _merge_forward(pkg, f"A merge ties (65, 63) joint={joint}", chans, near, far, t["merge", joint], joint)


# ---------------------------------------------------------------------------------------------------------------
# B. stage backward
# ---------------------------------------------------------------------------------------------------------------
def _merge_backward(pkg, dev, label, out, exp_low, Nc, near, far, dC_f, dmaps):
    bundle, _, _, perm, _ = out
    B = bundle.shape[0]
    ddist = _ddist(B)
    for with_colour in (True, False):
        dC = dC_f if with_colour else torch.zeros_like(dC_f)
        dm = dmaps if with_colour else None
        got = pkg.ops.merge_composite_backward_distortion(bundle, perm, dC.to(dev), Nc, near, far, ddist.to(dev), last=R.LAST,
                                                          dmaps=None if dm is None else dm.to(dev))
        ref64 = DR.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC, F64, near, far, ddist, dm)
        ref32 = DR.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC, F32, near, far, ddist, dm)
        low = DR.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC, F64, near, far, ddist, dm, exp_low=exp_low)
        bars = Bars(f"{label} colour+maps={with_colour}")
        for name, g, r64, r32, lo64 in zip(NAMES_D, got, ref64, ref32, low):
            assert bool(torch.isfinite(g).all()), (label, name, "an element was not written")  # (the outputs start as NaN)
            assert g.shape == r64.shape
            bars.add(name, g.cpu(), r64, r32, lo64)
        bars.check()
        if not with_colour:  # the distortion term alone: the colour branch receives exactly nothing
            assert bool((got[2] == 0).all()) and bool((got[3] == 0).all())
    # ddist = 0: the maps backward's values
    zero = pkg.ops.merge_composite_backward_distortion(bundle, perm, dC_f.to(dev), Nc, near, far, torch.zeros(B, 2, device=dev), last=R.LAST,
                                                       dmaps=dmaps.to(dev))
    maps = pkg.ops.merge_composite_backward(bundle, perm, dC_f.to(dev), Nc, last=R.LAST, dmaps=dmaps.to(dev))
    for name, a, b in zip(NAMES_D, zero, maps):
        assert torch.equal(a, b), (label, name)


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_merge_stage_backward(pkg, dev, Nc, Nf, joint):
    c = _case(pkg, dev, Nc, Nf)
    o = c["o"]
    _merge_backward(pkg, dev, f"B merge ({Nc}, {Nf}) joint={joint}", c["merge", joint], c["exp_low", joint], Nc, o["near"], o["far"], o["dC_f"],
                    o["dmaps"])


def test_merge_stage_backward_on_exact_ties(pkg, dev):
    t = _tie_case(pkg, dev)
    near, far = _tie_near_far(R.B_RAYS)
    _merge_backward(pkg, dev, "B merge ties (65, 63)", t["merge", 0], t["exp_low", 0], 65, near, far, t["o"]["dC_f"], t["o"]["dmaps"])


@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_coarse_stage_backward(pkg, dev, Nc, Nf):
    c = _case(pkg, dev, Nc, Nf)
    o, rep = c["o"], c["replica"]
    B = R.B_RAYS
    dt_f = torch.where(rep["ambiguous"], torch.zeros_like(o["dt_f"]), o["dt_f"])  # zeroed BEFORE both sides run, as in test_gpu_ray_stages E
    ddist = _ddist(B)
    # 8-ray buffers: rays 6, 7 are what the two waves behind the batch would touch if they stored anything
    pad = lambda x: torch.cat((x, x[:2]), 0).to(dev).contiguous()
    near8, far8 = torch.cat((o["near"], o["near"][:2])), torch.cat((o["far"], o["far"][:2]))
    SENTINEL = 123.0

    def run(rays, dC_c, dtf, dmaps, dd, calls=1, entry="dist"):
        dsig, drgb = torch.zeros(B + 2, Nc, device=dev), torch.zeros(B + 2, Nc, 3, device=dev)
        dsig[rays:] = SENTINEL
        drgb[rays:] = SENTINEL
        args = (pad(o["t_c"]), pad(o["sig_c"]), pad(o["rgb_c"]), near8, far8, o["delta0"], pad(dC_c), pad(dtf))
        dm = None if dmaps is None else pad(dmaps)
        for _ in range(calls):
            if entry == "dist":
                pkg.ops.coarse_composite_backward_distortion_add(*args, dsig, drgb, pad(dd), dmaps=dm, rays=rays)
            else:
                pkg.ops.coarse_composite_backward_add(*args, dsig, drgb, dmaps=dm, rays=rays)
        assert bool((dsig[rays:] == SENTINEL).all()) and bool((drgb[rays:] == SENTINEL).all()), f"{rays}-ray call stored behind its batch"
        return dsig[:rays], drgb[:rays]

    for with_colour in (True, False):
        oo = dict(o) if with_colour else dict(o, dC_c=torch.zeros_like(o["dC_c"]))
        dtf = dt_f if with_colour else torch.zeros_like(dt_f)
        dmaps = o["dmaps"] if with_colour else None
        ref64 = DR.coarse_grads(oo, rep["k"], F64, dtf, ddist, dmaps)
        ref32 = DR.coarse_grads(oo, rep["k"], F32, dtf, ddist, dmaps)
        low = DR.coarse_grads(oo, rep["k"], F64, dtf, ddist, dmaps, exp_low=c["exp_low"])
        dsig, drgb = run(B, oo["dC_c"], dtf, dmaps, ddist)
        assert bool(torch.isfinite(dsig).all()) and bool(torch.isfinite(drgb).all())
        bars = Bars(f"B coarse ({Nc}, {Nf}) colour+maps={with_colour}")
        bars.add("dsig_c", dsig.cpu(), ref64[0], ref32[0], low[0])
        bars.add("drgb_c", drgb.cpu(), ref64[1], ref32[1], low[1])
        bars.check()
        if not with_colour:
            assert bool((drgb == 0).all())
    dsig, drgb = run(B, o["dC_c"], dt_f, o["dmaps"], ddist)
    # "ADDS": a second call into the same buffers doubles them (g + g is exact)
    dsig2, drgb2 = run(B, o["dC_c"], dt_f, o["dmaps"], ddist, calls=2)
    assert torch.equal(_bits(dsig2), _bits(2 * dsig)) and torch.equal(_bits(drgb2), _bits(2 * drgb))
    # a 4-ray call (one full workgroup): the same bits for its rays
    dsig4, drgb4 = run(4, o["dC_c"], dt_f, o["dmaps"], ddist)
    assert torch.equal(_bits(dsig4), _bits(dsig[:4])) and torch.equal(_bits(drgb4), _bits(drgb[:4]))
    # ddist = 0: the maps backward's values
    z = run(B, o["dC_c"], dt_f, o["dmaps"], torch.zeros(B, 2))
    m = run(B, o["dC_c"], dt_f, o["dmaps"], None, entry="maps")
    assert torch.equal(z[0], m[0]) and torch.equal(z[1], m[1])


# ---------------------------------------------------------------------------------------------------------------
# C. whole call
# ---------------------------------------------------------------------------------------------------------------
def _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags):
    """nerf_hip_forward_distortion_train on a fresh workspace of exactly nerf_hip_ws_bytes -> (C_c, C_f, maps, dist, status, ws)"""
    _abi = pkg._abi
    dev = P[0].device
    B = row.shape[0]
    n = _abi.ws_bytes(B, Nc, Nf, flags)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    Cc, Cf = torch.full((B, 3), float("nan"), device=dev), torch.full((B, 3), float("nan"), device=dev)
    M, D = torch.full((B, 4), float("nan"), device=dev), torch.full((B, 2), float("nan"), device=dev)
    K9 = _abi.f32_array(K.reshape(-1).tolist())
    _abi.check(_abi.lib().nerf_hip_forward_distortion_train(_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, None, B, Nc, Nf,
                                                            pkg.nerf.LAST_DELTA, Cc.data_ptr(), Cf.data_ptr(), M.data_ptr(), ws.data_ptr(), n, flags,
                                                            torch.cuda.current_stream(dev).cuda_stream, D.data_ptr()))
    torch.cuda.synchronize()
    return Cc, Cf, M, D, _status(pkg, ws), ws


def _bwd_dist(pkg, P, ws, B, Nc, Nf, flags, dCc, dCf, dmaps, ddist):
    _abi = pkg._abi
    G = [torch.full_like(p, float("nan")) for p in P]
    _abi.check(_abi.lib().nerf_hip_backward_distortion(_abi.ptr_array(P), dCc.data_ptr(), dCf.data_ptr(), dmaps.data_ptr(), None, B, Nc, Nf,
                                                       pkg.nerf.LAST_DELTA, _abi.ptr_array(G), ws.data_ptr(), ws.numel(), flags,
                                                       torch.cuda.current_stream(P[0].device).cuda_stream, None, ddist.data_ptr()))
    torch.cuda.synchronize()
    return G


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_forward(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    N = Nc + Nf
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev)
    c0, f0, M0, s0, ws0 = _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")
    c1, f1, M1, D, s1, ws = _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags)
    assert ws.numel() == ws0.numel() == pkg._abi.ws_bytes(B, Nc, Nf, flags)  # the maps call's workspace: nothing per sample is saved
    assert torch.equal(c0, c1) and torch.equal(f0, f1) and torch.equal(M0, M1) and s0 == s1, mode
    view = lambda w, name, shape, dt=None: pkg._abi.ws_view(w, B, Nc, Nf, flags, name, shape, dt)
    assert torch.equal(view(ws, "bundle", (B, N, 5)), view(ws0, "bundle", (B, N, 5)))
    assert torch.equal(view(ws, "perm", (B, 5, N), torch.int16), view(ws0, "perm", (B, 5, N), torch.int16))
    near, far = pb[:, 15].double().cpu(), pb[:, 16].double().cpu()
    _assert_bar_a(f"C {mode} coarse", D[:, 0], DR.distortion(view(ws, "t_c", (B, Nc)).double().cpu(), view(ws, "w_c", (B, Nc)).double().cpu(), near, far))
    _assert_bar_a(f"C {mode} fine", D[:, 1],
                  DR.distortion(view(ws, "bundle", (B, N, 5))[:, :, 0].double().cpu(), view(ws, "w_m", (B, N)).double().cpu(), near, far))
    assert bool((D >= 0).all())


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_backward_with_zero_ddist_is_the_maps_backward(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev)
    gen = torch.Generator().manual_seed(11)
    dCc, dCf = (torch.randn(B, 3, generator=gen).to(dev) for _ in range(2))
    dmaps = torch.randn(B, 4, generator=gen).to(dev)
    ref = _bwd(pkg, P, _fwd(pkg, P, row, col, pb, K, Nc, Nf, flags, "train_maps")[4], B, Nc, Nf, flags, dCc, dCf, dmaps)
    got = _bwd_dist(pkg, P, _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags)[5], B, Nc, Nf, flags, dCc, dCf, dmaps, torch.zeros(B, 2, device=dev))
    for k, a, b in zip(_names(oracle), got, ref):
        assert torch.equal(a, b), (mode, k, float((a - b).abs().max()))


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_backward_fine_ray_stage_against_fp64(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    N = Nc + Nf
    _, P = _weights_dev(oracle, 1, False, dev)
    row, col, pb, K, _ = _inputs(oracle, B, dev, seed=5)
    ws = _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags)[5]
    view = lambda name, shape, dt=None: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, shape, dt)
    bundle = view("bundle", (B, N, 5)).double().cpu()
    perm = view("perm", (B, 5, N), torch.int16).long().cpu()
    g = _ddist(B, seed=7)
    zero3, zero4 = torch.zeros(B, 3, device=dev), torch.zeros(B, 4, device=dev)
    G = _bwd_dist(pkg, P, ws, B, Nc, Nf, flags, zero3, zero3, zero4, g.to(dev))
    t_s = bundle[:, :, 0]
    sig = bundle[:, :, 4].clone().requires_grad_(True)
    delta = torch.cat((t_s[:, 1:] - t_s[:, :-1], torch.full((B, 1), pkg.nerf.LAST_DELTA, dtype=F64)), 1)
    w = oracle.weights_from_sigma(delta, sig)
    (DR.distortion(t_s, w, pb[:, 15].double().cpu(), pb[:, 16].double().cpu()) * g[:, 1].double()).sum().backward()
    dsig = torch.zeros(B, N, dtype=F64).scatter_(1, perm[:, 4], sig.grad)
    got = view("dsig_f", (B, Nf)).double().cpu()
    e = l2_rel(got, dsig[:, Nc:])
    print(f"{mode}: d sigma_fine of the distortion term, L2-rel {e:.2e}")
    assert e < 3e-4, (mode, e)
    assert bool((view("drgb_c", (B, Nc, 3)) == 0).all()) and bool((view("drgb_f", (B, Nf, 3)) == 0).all())
    for k, q in zip(_names(oracle), G):
        assert torch.isfinite(q).all(), k
        if any(s in k for s in COLOUR_BRANCH):
            assert bool((q == 0).all()), (mode, k)


# ---------------------------------------------------------------------------------------------------------------
# D. Python
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_model_forward_distortion_under_autograd(oracle, pkg, dev, mode):
    flags, B = MODES[mode]
    Nc, Nf = 64, 128
    w, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K, Ct = _inputs(oracle, B, dev)
    m = _model(pkg, w, B, Nc, Nf, dev)
    _set_mode(m, flags)
    gen = torch.Generator().manual_seed(5)
    a, b = torch.randn(B, 3, generator=gen).to(dev), torch.randn(B, 3, generator=gen).to(dev)
    g, h = torch.randn(B, 4, generator=gen).to(dev), torch.randn(B, 2, generator=gen).to(dev)
    Cc, Cf, M, D = m(row, col, pb, K, maps=True, distortion=True)
    assert Cc.requires_grad and M.requires_grad and D.requires_grad and D.shape == (B, 2)
    ((Cc * a).sum() + (Cf * b).sum() + (M * g).sum() + (D * h).sum()).backward()
    got = [q.grad.clone() for q in m.network.parameters()]
    c1, f1, M1, D1, _, ws = _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags)
    assert torch.equal(Cc, c1) and torch.equal(Cf, f1) and torch.equal(M, M1) and torch.equal(D, D1)
    for k, x, y in zip(_names(oracle), got, _bwd_dist(pkg, P, ws, B, Nc, Nf, flags, a, b, g, h)):
        assert torch.equal(x, y), (mode, k)
    # a colour-only loss through it: forward's gradients (upstream gradients autograd hands over as None count as zero)
    m.zero_grad(set_to_none=True)
    Cc, Cf, M, D = m(row, col, pb, K, maps=True, distortion=True)
    m.ray_loss(Cc, Cf, Ct.to(dev)).backward()
    got = [q.grad.clone() for q in m.network.parameters()]
    m.zero_grad(set_to_none=True)
    Cc0, Cf0 = m(row, col, pb, K)
    m.ray_loss(Cc0, Cf0, Ct.to(dev)).backward()
    assert torch.equal(Cc, Cc0) and torch.equal(Cf, Cf0)
    for (k, q), x in zip(m.network.named_parameters(), got):
        assert torch.equal(x, q.grad), (mode, k)
    # distortion_loss alone (the colours' and the maps' upstream None): column 1 gets ones, column 0 zeros
    m.zero_grad(set_to_none=True)
    m.distortion_loss(m(row, col, pb, K, maps=True, distortion=True)[3]).backward()
    h1 = torch.zeros(B, 2, device=dev)
    h1[:, 1] = 1
    ref = _bwd_dist(pkg, P, _fwd_dist(pkg, P, row, col, pb, K, Nc, Nf, flags)[5], B, Nc, Nf, flags, torch.zeros_like(a), torch.zeros_like(b),
                    torch.zeros_like(g), h1)
    for (k, q), y in zip(m.network.named_parameters(), ref):
        assert torch.equal(q.grad, y), (mode, k)


def test_model_forward_distortion_bucket_and_refusals(oracle, pkg, dev):
    from nerf_tiny_amd import parallel as par

    w, _ = _weights_dev(oracle, 4, True, dev)
    B = 256
    row, col, pb, K, Ct = _inputs(oracle, B, dev)
    m = _model(pkg, w, B, 64, 128, dev)
    loss = lambda out: m.ray_loss(out[0], out[1], Ct.to(dev)) + 0.1 * m.distortion_loss(out[3], coarse=True)
    loss(m(row, col, pb, K, maps=True, distortion=True)).backward()
    ref = [q.grad.clone() for q in m.network.parameters()]
    bucket = par.GradBucket(m.network.parameters())
    m.grad_bucket = bucket
    try:
        loss(m(row, col, pb, K, maps=True, distortion=True)).backward()
        assert bucket.pending
        for q, v, r in zip(m.network.parameters(), bucket.views, ref):
            assert q.grad.data_ptr() == v.data_ptr() and torch.equal(v, r)
        bucket.consume()
    finally:
        m.grad_bucket = None
    first = loss(m(row, col, pb, K, maps=True, distortion=True))
    loss(m(row, col, pb, K, maps=True, distortion=True))  # a later training forward on the same workspace
    with pytest.raises(RuntimeError, match="reused by a later training forward"):
        first.backward()
    with pytest.raises(ValueError, match="maps=True"):
        m(row, col, pb, K, distortion=True)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"render\(quantiles=\)"):
            m(row, col, pb, K, maps=True, distortion=True)


def _runner(pkg, tmp, scene, dist_weight, mask_weight=0.0, iters=1):
    return pkg.NeRFRunner(gpu=0, img_dir="", results_path=str(tmp / "res") + "/", ckpt_path=str(tmp / "ck") + "/", low_res=1, total_iter=iters,
                          batch_ray=256, learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=100,
                          decay_end=10000, sched="EXP", datasets={"train": scene, "val": scene, "test": scene}, log_every=1,
                          on_resample_fault="ignore", distributed=False, mask_weight=mask_weight, dist_weight=dist_weight)


@pytest.mark.parametrize("mask_weight", [0.0, 0.5])
def test_runner_distortion_step_equals_the_hand_written_step(pkg, dev, tmp_path, mask_weight):
    from nerf_tiny_amd.train import regularized_train_step

    scene = pkg.data.analytic_sphere_scene(n_pic=3, H=24, W=24, device=str(dev))
    lam = 0.05
    torch.manual_seed(0)
    run = _runner(pkg, tmp_path / "a", scene, lam, mask_weight)
    losses = []
    run.writer.add_scalar = lambda tag, v, it: losses.append((tag, float(v)))
    assert run.trainer("train") == 0
    torch.manual_seed(0)
    hand = _runner(pkg, tmp_path / "b", scene, lam, mask_weight)
    m = hand.model
    row, col, pix, pb, pic, alpha = next(hand.train_rays.epoch(hand.batch_ray, with_alpha=True))
    _, _, loss = regularized_train_step(m, row, col, pb, hand.K_inv, pix, alpha if mask_weight > 0 else None, mask_weight, lam)
    hand.optimizer.step()
    for (k, a), b in zip(run.model.network.named_parameters(), m.network.parameters()):
        assert torch.equal(a, b), k
    assert [v for t, v in losses if t.startswith("loss/")] == [float(loss)]
    # the step's loss is what it says
    torch.manual_seed(0)
    m2 = _runner(pkg, tmp_path / "c", scene, lam, mask_weight).model
    Cc, Cf, M, D = m2(row, col, pb, hand.K_inv, maps=True, distortion=True)
    want = m2.ray_loss(Cc, Cf, pix) + (mask_weight * m2.mask_loss(M, alpha) if mask_weight > 0 else 0.0) + lam * D[:, 1].sum()
    assert float(want.detach()) == float(loss) and float(D[:, 1].sum().detach()) > 0


def test_runner_with_zero_dist_weight_takes_the_one_call_train_step(pkg, dev, tmp_path):
    scene = pkg.data.analytic_sphere_scene(n_pic=3, H=24, W=24, device=str(dev))
    torch.manual_seed(0)
    run = _runner(pkg, tmp_path / "a", scene, 0.0)
    losses = []
    run.writer.add_scalar = lambda tag, v, it: losses.append((tag, float(v)))
    assert run.trainer("train") == 0
    torch.manual_seed(0)
    hand = _runner(pkg, tmp_path / "b", scene, 0.0)
    row, col, pix, pb, pic = next(hand.train_rays.epoch(hand.batch_ray))
    hand.model.grad_bucket = hand.bucket
    try:
        _, _, loss = hand.model.train_step(row, col, pb, hand.K_inv, pix)
    finally:
        hand.model.grad_bucket = None
    hand.optimizer.step()
    for (k, a), b in zip(run.model.network.named_parameters(), hand.model.network.parameters()):
        assert torch.equal(a, b), k
    assert [v for t, v in losses if t.startswith("loss/")] == [float(loss)]


def _run_ranks(n, out, extra=(), timeout=300):
    import socket

    tool = os.path.join(ROOT, "tests", "tools", "dist_runner_rank.py")
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
    assert "DIST-RUNNER-OK" in r.stdout
    return torch.load(os.path.join(out, "result.pt"), weights_only=False)


@pytest.mark.timeout(600)
def test_distortion_runner_single_rank_rccl_equals_plain_runner(tmp_path):
    plain = _run_ranks(0, str(tmp_path / "plain"))
    dp = _run_ranks(1, str(tmp_path / "dp1"), ("--force-dist",))
    assert plain["distributed"] is False and dp["distributed"] is True and dp["ranks"] == 1
    assert len(dp["losses"]) == 3
    assert plain["losses"] == dp["losses"]
    assert torch.equal(plain["weights"], dp["weights"])
