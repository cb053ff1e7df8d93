"""GPU: the two ends of the field that the layer suites take as given, held to restatements of their own operands.

tests/test_gpu_layers.py checks every layer between gamma_p and g0 from operands it reads out of the workspace; what PRODUCES the first
of them (ray records, depths, sample points, the sin / cos of 3,217 rad per unit, the fold) and what CONSUMES the last (d gamma_p -> d point
-> d t_fine, fine pass only) is checked here, per arithmetic of test_gpu_layers.ARITHS, at (B, Nc, Nf) = (2, 2, 1), (7, 5, 3), (50, 24, 40),
(130, 31, 65), (3, 1024, 1024): the ABI's minimum, rows that are no multiple of 32 / 64 / 256, ray boundaries inside a wave with the lanes
behind the batch clamped to row M - 1, the maximum.  Inputs: tests/field_ends_reference.py field_ends_inputs (the fern fixture with a
translation per ray chosen for the phase classes of coverage(); asserted on the case's own rows before the device is looked at, as far as
a case of its size can hold them: test_field_ends_cpu.coverage_wanted), a seeded sharp state dict, and the autograd entry with seeded
upstream gradients, ((C_c * a).sum() + (C_f * b).sum()).backward(), so that dC_c = a and dC_f = b exactly.

A. Forward end, no tolerance.  rayf[:, :22] and t_c equal ray_record / coarse_depth of (row, col, pose, K^-1) bit for bit; the saved gamma_p
rows of both passes (64 columns, the zero padding included) equal gamma_p(rayf, t) of the device's own rayf, t_c, t_f bit for bit (fp32,
fp32_tile), its RNE-bf16 (bf16_mlp), hi = RNE(v) and mid = RNE(v - hi) (split_train); ops.field(debug=True) gives the same points and
encodings.  gamma_d: bf16_mlp / split_train take it through sincos_phase (bit equality through their rounding); fp32 / fp32_tile call the
device library's sinf / cosf (gdbuf), held to the 1 ulp HIP documents for both against float64 of the fp32 phase (one fp32 step from the
correctly rounded value: the integer distance HIP's table lists, hence at most 1.5 ulp from the exact value, also asserted.  This is not
the reading of test_gpu_ray_stages._exp_low, which holds expf to 1.0 ulp of the exact value: the library's sinf measures 1.24 there).
dvec against b_dir + W_dir[:, :24] gamma_d + b_fold of the device's own gdbuf and b_fold, fold / b_fold against float64 products of the parameters, at
test_gpu_layers.E_FP32 of the magnitude (one k-ordered fp32 accumulation each).

B. Output end.  The merge backward is called once more on the workspace's own bundle / perm with dC_f = b (it reproduces the step's
dsig_f / drgb_f bit for bit: the same stage; no size here is the fused small-batch bf16 form, which needs (64, 128)); its dt is dt_merge.
The workspace's final dt_f is held to
    |dt_f - (dt_merge + dt_field64)| <= (s E + 2^-20) mag_dt + 2^-24 |dt_f|        (field_ends_reference.dt_field, dt_bar)
with E the mode's constant and s = 1 in every kernel: field_bwd.hip (accg: SEG_T_L4B then SEG_T_L0), field_bwd_reg.hip (accg: the two thin
layers), field_bwd_bf16.hip and field_bwd_split.hip (BSEG_G0T: "in the same accumulator") all run W_4[:, 256:]^T g4 and W_0^T g0 into one
accumulator.  With b = 0 the fine pass leaves dt_f exactly zero, and the bytes behind dt_f's B Nf elements stay as they were poisoned.

Measured on the MI355X, worst |dt_f - (dt_merge + dt_field64)| / bar (printed by the test):
    (B, Nc, Nf)        fp32    fp32_tile   bf16_mlp   split_train
    (2, 2, 1)          0.000   0.002       0.008      0.001
    (7, 5, 3)          0.070   0.049       0.011      0.013
    (50, 24, 40)       0.110   0.110       0.322      0.518
    (130, 31, 65)      0.195   0.190       0.489      0.186
    (3, 1024, 1024)    0.580   0.506       0.082      0.306
The bar exceeds half of |dt_field64| on at most 0.07 % of the elements; the field's part is 84-98 % of sum |dt_f| (29 % at 1,024 samples).
Forward end, x E_FP32 of the magnitude: b_fold 0.063, fold 0.082, dvec 0.074-0.266; gdbuf one fp32 step from the correctly rounded value at
most (1.24 ulp, 0.94 x 2^-24 from the exact one).  Every bit equality held: no exception is written down.  A coordinate that is exactly
-0 (a rotation row of signed zeros) encodes to sines of -0, as libm's sin does: the last test.

Out of reach: the fused small-batch bf16 backward (csrc/api.hip fuse_rays: Nc = 64, Nf = 128 only), where the merge backward runs inside the
field launch and dt[m] += follows it in one kernel -- no size here reaches it and the stage call cannot reproduce its dt_merge separately;
and the inference-only encode sites, which store no encodings -- field_fwd_bf16x.hip (its written-out copy of encode_pair), the pair
renderer, and the query form of field_fwd_reg.hip beyond what test_query_is_bit_identical_to_the_ray_path ties to the ray path.  They
stay checked end to end against the emulation only; a debug output for them would be an ABI change.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import field_ends_reference as F
import ws_operands as W
from test_field_ends_cpu import SIZES, coverage_wanted
from test_gpu_layers import ARITHS, E_BF16, E_FP32, MODE, _flags, _model, _over

pytestmark = pytest.mark.gpu

TRAIN_STEP_SIZE = (130, 31, 65)
ULP_SINF = 1.0  # HIP math API, single precision: sinf and cosf are listed with an ULP difference of 1 to the host's double result
CASES = [pytest.param(a, *s, id=f"{a}-{s[0]}x{s[1]}+{s[2]}") for a in ARITHS for s in SIZES]


@functools.lru_cache(maxsize=None)
def _inputs(B, Nc):
    import nerf_oracle

    return F.field_ends_inputs(nerf_oracle, B, Nc)


def _bits(name, got, want):
    """fp32 tensors, bit for bit; the first differing element is named."""
    g, w = got.contiguous().view(torch.int32).cpu(), want.contiguous().view(torch.int32).cpu()
    assert g.shape == w.shape, (name, g.shape, w.shape)
    ne = (g != w).flatten()
    if bool(ne.any()):
        i = int(ne.nonzero()[0])
        raise AssertionError(f"{name}: {int(ne.sum())} of {ne.numel()} elements differ; first at flat index {i}: device "
                             f"{float(got.flatten()[i]):.9g} (0x{int(g.flatten()[i]) & 0xffffffff:08x}), restated "
                             f"{float(want.flatten()[i]):.9g} (0x{int(w.flatten()[i]) & 0xffffffff:08x})")


def _ordered(x):
    """fp32 -> int64 that counts fp32 steps along the real line."""
    i = x.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _rounded(name, mode, parts, want32):
    """The saved operand `parts` against the fp32 values want32 through the mode's rounding."""
    v = want32.double().to(parts[0].device)
    if mode == "fp32":
        _bits(name, parts[0], want32.to(parts[0].device))
        return
    hi = W.rne_bf16(v)
    bad = parts[0].double() != hi
    assert not bool(bad.any()), (name, "hi", int(bad.sum()), int(bad.flatten().nonzero()[0]))
    if mode == "split":
        bad = parts[1].double() != W.rne_bf16(v - hi)
        assert not bool(bad.any()), (name, "mid", int(bad.sum()), int(bad.flatten().nonzero()[0]))


def _gp64(ws, B, Nc, Nf, flags, mode):
    """The saved gamma_p rows with their padding: parts [B (Nc + Nf), 64], coarse rows then fine rows."""
    from nerf_tiny_amd import _abi

    if mode == "fp32":
        Mtot = B * (Nc + Nf)
        save = _abi.ws_view(ws, B, Nc, Nf, flags, "save", (W.NSAVE, Mtot + W.DUMP_ROWS, W.WIDTH))
        return (save[W.S_GP, :Mtot, :F.GP_COLS],)
    _, wb_tot, ranges = W.pass_rows(B, Nc, Nf)
    out = []
    for name in ("bsave",) if mode == "bf16" else ("bsave", "bsave2"):
        buf = _abi.ws_view(ws, B, Nc, Nf, flags, name, (wb_tot * sum(W.BS_KS) * W.FRAG_BYTES,), torch.uint8)
        out.append(W._real(W.decode(buf, wb_tot, W.BS_KS, W.BS_GP), ranges))
    assert all(t.shape[1] == F.GP_COLS for t in out)
    return tuple(out)


def _run(pkg, dev, arith, B, Nc, Nf, entry, fine_upstream=True):
    """One step; -> everything the checks read, and the guard region's verdict."""
    import nerf_oracle
    from nerf_tiny_amd import _abi

    row, col, pb, K, Ct = _inputs(B, Nc)
    m = _model(pkg, nerf_oracle.make_weights(6, sharp=True), arith, B, Nc, Nf, dev)
    flags = _flags(arith)
    view = lambda name, shape, dt=None: _abi.ws_view(m.last_workspace, B, Nc, Nf, flags, name, shape, dt)
    gen = torch.Generator().manual_seed(11)
    a = torch.randn(B, 3, generator=gen).to(dev)
    b = (torch.randn(B, 3, generator=gen) if fine_upstream else torch.zeros(B, 3)).to(dev)
    guard = None
    if entry == "autograd":
        ws = m._workspace(B, flags)
        off = ctypes.c_size_t(0)
        _abi.check(_abi.lib().nerf_hip_ws_offset(B, Nc, Nf, flags, b"dt_f", ctypes.byref(off)))
        first = off.value + B * Nf * 4
        guard = ws[first:]
        assert guard.numel() >= B * 9 * 4  # dC, which only nerf_hip_train_step writes, and the alignment padding in front of it
        guard.fill_(0xA5)
        Cc, Cf = m(row, col, pb, K)
        assert m.last_workspace.data_ptr() == ws.data_ptr()
        ((Cc * a).sum() + (Cf * b).sum()).backward()
    else:
        m.train_step(row, col, pb, K, Ct)
    torch.cuda.synchronize()
    c = {"m": m, "flags": flags, "view": view, "a": a, "b": b, "inputs": (row, col, pb, K), "mode": MODE[arith], "sizes": (B, Nc, Nf)}
    c["guard_ok"] = None if guard is None else bool((guard == 0xA5).all())
    c["rayf"], c["t_c"], c["t_f"] = view("rayf", (B, F.RAYF)), view("t_c", (B, Nc)), view("t_f", (B, Nf))
    return c


def _coverage(c):
    B, Nc, Nf = c["sizes"]
    rf = c["rayf"].cpu().numpy()
    p = np.concatenate((F.sample_point(rf, c["t_c"].cpu().numpy()).reshape(-1, 3), F.sample_point(rf, c["t_f"].cpu().numpy()).reshape(-1, 3)))
    cov = F.coverage(p)
    assert cov["max_abs"] <= 320.0, cov
    for k, v in coverage_wanted(B, Nc, Nf).items():
        assert cov[k] >= v, (k, cov)
    return cov


def _forward_end(c, pkg, dev):
    B, Nc, Nf = c["sizes"]
    row, col, pb, K = c["inputs"]
    mode, view, m = c["mode"], c["view"], c["m"]
    ws = m.last_workspace
    weights = [p.detach() for p in m.network.parameters()]
    # rays and depths from (row, col, pose, K^-1)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    _bits("rayf[:, :22]", c["rayf"][:, :22], torch.from_numpy(rf[:, :22]))
    _bits("t_c", c["t_c"], torch.from_numpy(F.coarse_depth(rf, Nc)))
    # gamma_p of both passes from the device's own rayf, t_c, t_f
    rfd = c["rayf"].cpu().numpy()
    want = torch.from_numpy(np.concatenate((F.gamma_p(rfd, c["t_c"].cpu().numpy()), F.gamma_p(rfd, c["t_f"].cpu().numpy()))))
    _rounded("gamma_p", mode, _gp64(ws, B, Nc, Nf, c["flags"], mode), want)
    ray = torch.cat((torch.arange(B * Nc) // Nc, torch.arange(B * Nf) // Nf))
    ops = W.read_operands(ws, B, Nc, Nf, c["flags"])
    out = {}
    Wd, Wpi, bpi, bd = (weights[i].double() for i in (W.W_DIR, W.W_PI, W.B_PI, W.B_DIR))
    fold = view("fold", (W.HALF + W.HALF * W.WIDTH,))
    b_fold = fold[:W.HALF].double()
    r = (b_fold - Wd[:, W.DIR_DIM:] @ bpi).abs() / (E_FP32 * (Wd[:, W.DIR_DIM:].abs() @ bpi.abs()))
    out["b_fold"] = float(r.max())
    Wf = fold[W.HALF:].view(W.HALF, W.WIDTH).double()  # every mode: the fp32 packer builds SEG_FOLD from the same fold kernel's output
    r = (Wf - Wd[:, W.DIR_DIM:] @ Wpi).abs() / (E_FP32 * (Wd[:, W.DIR_DIM:].abs() @ Wpi.abs()))
    out["fold"] = float(r.max())
    if mode == "fp32":
        gdbuf = view("gdbuf", (B, W.DIR_DIM)).double()
        ref = torch.from_numpy(F.gamma_d(rfd[:, F.RF_DWRD:F.RF_DWRD + 3], "libm")).to(dev)
        # HIP documents sinf / cosf by the distance, in fp32 steps, between the device's result and the host's double result as an fp32:
        # 1.  So the device value is the correctly rounded one or a neighbour, which is at most 1.5 ulp from the exact value; both figures
        # are asserted.  (Measured 1.24 ulp, 0.94 x 2^-24 absolute -- the library's own sinf: torch.sin on the device gives the same bits.
        # This reading differs from test_gpu_ray_stages._exp_low, which holds expf to 1.0 ulp of the EXACT value: sinf does not meet that.)
        steps = (_ordered(gdbuf.float()) - _ordered(ref.float())).abs()
        ulp = W.pow2(torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1].to(torch.int64) - 24)  # spacing of fp32 at |ref|
        out["gdbuf steps"] = float(steps.max())
        out["gdbuf ulps"] = float(((gdbuf - ref).abs() / ulp).max())
        out["gdbuf abs / 2^-24"] = float((gdbuf - ref).abs().max()) * 2.0 ** 24
        assert out["gdbuf steps"] <= ULP_SINF and out["gdbuf ulps"] <= ULP_SINF + 0.5, out
        dvec = view("dvec", (B, W.HALF)).double()
        Wg = Wd[:, :W.DIR_DIM]
        ref = bd + gdbuf @ Wg.T + b_fold
        mag = bd.abs() + gdbuf.abs() @ Wg.abs().T + b_fold.abs()
        out["dvec"] = float(((dvec - ref).abs() / (E_FP32 * mag)).max())
    else:
        gd = torch.from_numpy(F.gamma_d(rfd[:, F.RF_DWRD:F.RF_DWRD + 3], "phase"))[ray]
        _rounded("gamma_d", mode, ops["gd"], gd)
    for k, v in out.items():
        if not k.startswith("gdbuf"):
            assert v <= 1.0, (k, out)
    return out


def _output_end(c, pkg):
    B, Nc, Nf = c["sizes"]
    mode, view, m = c["mode"], c["view"], c["m"]
    ws = m.last_workspace
    weights = [p.detach() for p in m.network.parameters()]
    ops = W.read_layer_operands(ws, B, Nc, Nf, c["flags"])
    bundle, perm = view("bundle", (B, Nc + Nf, 5)), view("perm", (B, 5, Nc + Nf), torch.int16)
    _, dsig_f, _, drgb_f, dt_merge = pkg.ops.merge_composite_backward(bundle, perm, c["b"], Nc)
    _bits("dsig_f of the merge backward", dsig_f.reshape(-1), view("dsig_f", (B * Nf,)))
    _bits("drgb_f of the merge backward", drgb_f.reshape(-1), view("drgb_f", (B * Nf * 3,)))
    fine = lambda parts: tuple(t[B * Nc:] for t in parts)
    R = W.reference_weights(ops, weights, mode)
    dt64, mag = F.dt_field(fine(ops["g0"]), fine(ops["g4"]), R, c["rayf"].cpu().numpy(), c["t_f"].cpu().numpy())
    dt_f = view("dt_f", (B * Nf,)).double()
    E = E_FP32 if mode == "fp32" else E_BF16
    bar = F.dt_bar(mag, dt_f, E)
    err = (dt_f - (dt_merge.reshape(-1).double() + dt64)).abs()
    ratio = _over(err, bar)
    i = int(ratio.argmax())
    vac = float((bar > 0.5 * dt64.abs()).double().mean())
    dead = float((mag == 0).double().mean())
    return {"worst": float(ratio[i]), "at": (i // Nf, i % Nf), "vacuous": vac, "dead": dead, "dt_f": float(dt_f[i]), "dt_field": float(dt64[i]),
            "field_share": float(dt64.abs().sum() / dt_f.abs().sum().clamp_min(1e-300))}


@pytest.mark.parametrize("arith,B,Nc,Nf", CASES)
def test_field_ends_against_their_restatements(pkg, dev, arith, B, Nc, Nf):
    c = _run(pkg, dev, arith, B, Nc, Nf, "autograd")
    cov = _coverage(c)
    fwd = _forward_end(c, pkg, dev)
    end = _output_end(c, pkg)
    print(f"\n{arith} {B}x({Nc}+{Nf}): coverage {cov}; forward end (x bar) {', '.join(f'{k} {v:.3f}' for k, v in fwd.items())}; output end worst "
          f"{end['worst']:.3f} x bar at ray {end['at'][0]} sample {end['at'][1]} (dt_f {end['dt_f']:.4g}, field part {end['dt_field']:.4g}); "
          f"bar above half the field part on {100 * end['vacuous']:.2f} % of the elements; rows with no gradient {100 * end['dead']:.1f} %; "
          f"sum |field part| / sum |dt_f| {end['field_share']:.3g}")
    assert end["worst"] <= 1.0, end
    assert end["vacuous"] < 0.10, end
    assert c["guard_ok"], "bytes behind dt_f were written"


@pytest.mark.parametrize("arith", ARITHS)
def test_forward_end_of_the_train_step(pkg, dev, arith):
    c = _run(pkg, dev, arith, *TRAIN_STEP_SIZE, "train_step")
    _coverage(c)
    fwd = _forward_end(c, pkg, dev)
    print(f"\n{arith} train_step: forward end (x bar) {', '.join(f'{k} {v:.3f}' for k, v in fwd.items())}")


@pytest.mark.parametrize("arith", ARITHS)
def test_the_coarse_colour_leaves_no_position_gradient(pkg, dev, arith):
    """b = 0: dC_f = 0, so the merge backward and the fine chain add nothing, and the coarse pass has no path to t_fine."""
    B, Nc, Nf = 50, 24, 40
    c = _run(pkg, dev, arith, B, Nc, Nf, "autograd", fine_upstream=False)
    assert not bool(c["view"]("dt_f", (B * Nf,)).view(torch.int32).any()) and c["guard_ok"]


@pytest.mark.parametrize("B,Nc,Nf", SIZES)
def test_debug_outputs_of_the_field_call(pkg, dev, B, Nc, Nf):
    """ops.field(debug=True) (k_field_fwd_reg<DEBUG>): points and encodings of the coarse depths, bit for bit."""
    import nerf_oracle

    row, col, pb, K, _ = _inputs(B, Nc)
    m = _model(pkg, nerf_oracle.make_weights(6, sharp=True), "fp32", B, Nc, Nf, dev)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    t = F.coarse_depth(rf, Nc)
    _, _, pts, gp = pkg.ops.field([p.detach() for p in m.network.parameters()], row.to(dev), col.to(dev), pb.to(torch.float32).to(dev), K,
                                  torch.from_numpy(t).to(dev), debug=True)
    _bits("pts", pts, torch.from_numpy(F.sample_point(rf, t)))
    _bits("gamma_p", gp.reshape(-1, 60), torch.from_numpy(F.gamma_p(rf, t)[:, :60]))


def test_a_negative_zero_coordinate_keeps_its_sign(pkg, dev):
    """sin(-0) = -0 on the device.  Row 1 of ray 0's rotation is zeros signed against d_cam and its translation is -0, so every product
    and sum of sample_point is -0 and the coordinate is -0 at every sample: its ten sines are -0 (0x80000000), its cosines 1, and the call's
    points and encodings equal the restatement bit for bit."""
    import nerf_oracle

    B, Nc, Nf = 7, 5, 3
    row, col, pb, K, _ = _inputs(B, Nc)
    pb = pb.clone()
    d_cam = F.ray_record(row, col, pb.to(torch.float32), K, Nc)[0, F.RF_DCAM:F.RF_DCAM + 3]
    for k in range(3):
        pb[0, 5 + k] = -0.0 if d_cam[k] > 0 else 0.0  # times d_cam[k] * t, t > 0: -0
    pb[0, 5 + 3] = -0.0
    m = _model(pkg, nerf_oracle.make_weights(6, sharp=True), "fp32", B, Nc, Nf, dev)
    rf = F.ray_record(row, col, pb.to(torch.float32), K, Nc)
    t = F.coarse_depth(rf, Nc)
    want_p, want_g = F.sample_point(rf, t), F.gamma_p(rf, t)[:, :60]
    assert (want_p[0, :, 1].view(np.uint32) == 0x80000000).all() and (want_g[:Nc, 20:40:2].view(np.uint32) == 0x80000000).all()
    _, _, pts, gp = pkg.ops.field([p.detach() for p in m.network.parameters()], row.to(dev), col.to(dev), pb.to(torch.float32).to(dev), K,
                                  torch.from_numpy(t).to(dev), debug=True)
    _bits("pts", pts, torch.from_numpy(want_p))
    _bits("gamma_p", gp.reshape(-1, 60), torch.from_numpy(want_g))
    assert bool((gp[0, :, 21:40:2] == 1).all())
