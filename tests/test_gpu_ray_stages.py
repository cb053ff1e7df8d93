"""GPU: the per-ray stages between the MLP and the loss -- coarse weights + inverse-CDF resampling, the five channel sorts + merged composite,
and the backward of each (ray_parts.h, ray_parts_bwd.h, ray_ops.hip, ray_ops_bwd.hip) -- through their stage entry points, against float64 of
their own operands (tests/ray_stage_reference.py), at every size at which the kernels take another path.

  A. coarse forward: w_c, C_c, t_f, the maps columns 0, 1; the status bit exactly where the decision replica raises the Q7 condition;
  B. the training sort (k_merge<true>): perm is THE stable permutation of every channel (torch.sort's order: +-0 equal, NaNs last, padding
     behind real NaNs), the bundle is its gather, joint = 0 gives the values-only kernel's bits, joint = 1 the depth order five times;
  C. merged composite forward: w, C_f, the maps columns 2, 3 over the device's own sorted bundle;
  D. merge backward: all five gradients, without and with dmaps; every element written; dC_f = 0 leaves the rgb gradients exactly zero;
  E. coarse backward: d sigma_c, d rgb_c without and with dmaps; the ADD contract; nothing stored for the waves behind the batch.

Bars: nothing is fixed in advance.  Per case and tensor the same graph runs once more in torch float32 on the CPU with the same bins / sort
order; e32 = its L2-rel distance to float64.  The bar first was max(2.5 e32, 1e-6) (2.5: the margin of
test_every_gradient_is_as_accurate_as_the_reference, for the device's expf and another summation order; 1e-6, about 16 fp32 ulps, for tensors
the CPU happens to get almost exactly).  Elementwise tensors meet it at every size (<= 1.6 e32) and everything does up to (128, 128) (<= 2.4),
but the tensors that SUM over a ray's samples -- C, D, A, d sigma -- measured 3.1-4.5 e32 at N = 330 and 12.6-18.3 e32 at N = 2048.  The cause
 is not the kernels' arithmetic: the device's expf, inside its documented 1 ulp, comes out 0.08-0.12 ulp LOW on average for
results just below 1, where the CPU's averages to ~0; 1 - expf(-s) makes that a same-sign error of every weight, and a sum collects it N-fold
where unbiased rounding collects sqrt(N)-fold.  So the bar carries that mechanism, not a wider margin: the test measures how low the device's
own exp comes out on the case's own arguments (per ray, mean signed error in units of 2^-24, asserted within 1), evaluates the float64 graph
once more with exp(-s) that much low (R.weights(exp_low=)), calls that tensor's shift e_exp, and holds the device to
max(2.5 (e32 + e_exp), 1e-6).  Measured: 0.10-1.40 of e32 + e_exp over all sizes and tensors (0.92-0.99 where the bias dominates: the model
accounts for all of the excess).  Each test prints both ratios; DESIGN.md section 6z lists them per size.
Bit-equality, permutation and status assertions take no tolerance.

Sizes (Nc, Nf), 6 rays each (the last k_coarse / k_coarse_bwd workgroup has two waves behind the batch):
  (2, 1) the ABI's minimum; (5, 3) N = P = 8, Nc > Nf: the Q7 bit must be set and t_f still match the clamped reference; (31, 65) N = 96,
  P = 128; (65, 63) one lane into the second coarse chunk, the LDS network without padding; (64, 65) N = 129: the register network with 127
  padding slots; (64, 128) the shipped size; (128, 128) the register network without padding, Nc exactly two chunks; (130, 200) P = 512, a
  ragged third chunk on both sides; (1024, 1024) the maximum (k_coarse_bwd: 88 KiB of dynamic LDS, k_merge<true>: 60 KiB).
"""
import pytest
import torch

import ray_stage_reference as R

pytestmark = pytest.mark.gpu

SIZES = list(R.CASES)
MARGIN, FLOOR = 2.5, 1e-6
F32, F64 = torch.float32, torch.float64


class Bars:
    """collects (device error, fp32 error) per tensor of one test and asserts the bar at the end, after printing every figure"""

    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, name, got, ref64, ref32, low64):
        """low64: the float64 graph with exp(-s) as low as the device's exp measures on this case's own arguments (R.weights, _exp_low)"""
        e, e32, eexp = R.l2_rel(got, ref64), R.l2_rel(ref32, ref64), R.l2_rel(low64, ref64)
        self.rows.append((name, e, e32, eexp, e / max(e32 + eexp, FLOOR / MARGIN), e / max(e32, FLOOR / MARGIN)))

    def check(self):
        worst = max(self.rows, key=lambda r: r[4])
        print(f"{self.label}: worst ratio {worst[4]:.2f} ({worst[0]}: device {worst[1]:.2e}, fp32 {worst[2]:.2e}, exp bias {worst[3]:.2e}); "
              "device / (fp32 + exp bias) [device / fp32 alone]: " + ", ".join(f"{n} {r:.2f} [{r0:.2f}]" for n, _, _, _, r, r0 in self.rows))
        for n, e, e32, eexp, r, r0 in self.rows:
            assert e <= max(MARGIN * (e32 + eexp), FLOOR), (self.label, n, e, e32, eexp)


def _exp_low(dev, s32):
    """R.exp_low_of for the DEVICE's exp on the case's own arguments s32 [B,N] (fp32, as the kernel forms them), taken with torch.exp on the
    device -- the device library's expf, which the kernels call too: the summed errors of the kernels' own weights match the bias measured
    this way.  Its size is held to the 1 ulp HIP documents for expf, so a kernel error cannot hide in it."""
    m = R.exp_low_of(torch.exp(-s32.to(dev)).cpu(), s32)
    assert float(m.abs().max()) <= 1.0, m
    return m


def _merge_s32(bundle):
    b = bundle.cpu()
    delta = torch.cat((b[:, 1:, 0] - b[:, :-1, 0], torch.full((b.shape[0], 1), R.LAST)), dim=1)
    return delta * b[:, :, 4]


_CASES = {}


def _case(pkg, dev, Nc, Nf):
    """everything the tests of one size share, computed once: the operands, the coarse forward on the device, the decision replica on the
    device's own w_c, the training sorts of the device's own t_f"""
    if (Nc, Nf) in _CASES:
        return _CASES[(Nc, Nf)]
    o = R.operands(Nc, Nf)
    d = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in o.items()}
    c = dict(o=o, d=d)
    c["coarse"] = pkg.ops.coarse_composite_maps(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], Nf)
    w_c, _, t_f, _, _ = c["coarse"]
    c["replica"] = R.decision_replica(w_c.cpu(), Nf)
    c["exp_low"] = _exp_low(dev, ((o["far"] - o["near"]) / Nc)[:, None] * o["sig_c"])
    for joint in (0, 1):
        c["merge", joint] = pkg.ops.merge_composite_train(d["t_c"], t_f, d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"], last=R.LAST,
                                                          joint=bool(joint), maps=True)
        c["exp_low", joint] = _exp_low(dev, _merge_s32(c["merge", joint][0]))
    _CASES[(Nc, Nf)] = c
    return c


_TIES = {}


def _tie_case(pkg, dev):
    if not _TIES:
        o = R.tie_operands()
        d = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in o.items()}
        _TIES.update(o=o, d=d)
        for joint in (0, 1):
            _TIES["merge", joint] = pkg.ops.merge_composite_train(d["t_c"], d["t_f"], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"], last=R.LAST,
                                                                  joint=bool(joint), maps=True)
            _TIES["exp_low", joint] = _exp_low(dev, _merge_s32(_TIES["merge", joint][0]))
    return _TIES


def _bits(x):
    return x.contiguous().view(torch.int32)


def _channels(t_c, t_f, sig_c, sig_f, rgb_c, rgb_f):
    """[B,5,N] on the CPU: channel 0 = t, 1..3 = rgb, 4 = sigma; coarse slots first"""
    t, sg, rgb = torch.cat((t_c, t_f), 1), torch.cat((sig_c, sig_f), 1), torch.cat((rgb_c, rgb_f), 1)
    return torch.stack((t, rgb[:, :, 0], rgb[:, :, 1], rgb[:, :, 2], sg), dim=1).cpu()


def _same_values(a, b):
    """value-equal with NaN positions equal (a -0 and a +0 are the same value)"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ---------------------------------------------------------------------------------------------------------------
# A. coarse forward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_coarse_forward_against_fp64(pkg, dev, Nc, Nf):
    c = _case(pkg, dev, Nc, Nf)
    o, d, rep = c["o"], c["d"], c["replica"]
    w_c, C_c, t_f, status, maps = c["coarse"]
    amb = rep["ambiguous"]
    print(f"({Nc}, {Nf}): {int(amb.sum())} of {amb.numel()} fine samples ambiguous on the device's w_c")
    assert int(amb.sum()) <= R.AMBIGUOUS_MAX * amb.numel()
    with torch.no_grad():
        s64 = R.coarse_stage(o["sig_c"].double(), o["rgb_c"].double(), o["t_c"], o["near"], o["far"], o["delta0"], Nf, rep["k"])
        s32 = R.coarse_stage(o["sig_c"], o["rgb_c"], o["t_c"], o["near"], o["far"], o["delta0"], Nf, rep["k"])
        low = R.coarse_stage(o["sig_c"].double(), o["rgb_c"].double(), o["t_c"], o["near"], o["far"], o["delta0"], Nf, rep["k"], c["exp_low"])
    bars = Bars(f"A ({Nc}, {Nf})")
    for name, got in (("w", w_c), ("C_c", C_c), ("t_f", t_f), ("D_c", maps[:, 0]), ("A_c", maps[:, 1])):
        assert bool(torch.isfinite(got).all()), name
        bars.add(name, got.cpu(), s64[name], s32[name], low[name])
    assert bool(torch.isnan(maps[:, 2:]).all())  # the fine maps' columns are not this kernel's
    # k_coarse (no maps): the same bits
    w0, C0, t0, st0 = pkg.ops.coarse_composite(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], Nf)
    assert torch.equal(_bits(w0), _bits(w_c)) and torch.equal(_bits(C0), _bits(C_c)) and torch.equal(_bits(t0), _bits(t_f)) and st0 == status
    # the status bit (quirk Q7): set exactly where the replica's unclamped bin leaves [0, Nf-1] -- for the call, and ray by ray
    assert (status & 1) == int(bool(rep["bad"].any()))
    if (Nc, Nf) == (5, 3):
        assert status & 1
    for b in range(R.B_RAYS):
        w1, C1, t1, st1 = pkg.ops.coarse_composite(d["t_c"][b:b + 1], d["sig_c"][b:b + 1], d["rgb_c"][b:b + 1], o["near"][b:b + 1],
                                                   o["far"][b:b + 1], o["delta0"], Nf)
        assert (st1 & 1) == int(bool(rep["bad"][b].any())), b
        assert torch.equal(_bits(t1[0]), _bits(t_f[b])) and torch.equal(_bits(w1[0]), _bits(w_c[b])), b
    bars.check()


# ---------------------------------------------------------------------------------------------------------------
# B. the training sort
# ---------------------------------------------------------------------------------------------------------------
def _check_sort(pkg, chans, out, joint, Nc):
    """chans [B,5,N] (CPU): what went in; out: merge_composite_train's result"""
    bundle, w, C_f, perm, _ = out
    perm = perm.long().cpu()
    want = R.stable_order(chans)
    if joint:
        want = want[:, 0:1].expand(-1, 5, -1)
    assert torch.equal(perm, want), f"joint={joint}: {int((perm != want).sum())} permutation entries differ"
    assert _same_values(bundle.cpu().permute(0, 2, 1), torch.gather(chans, 2, perm))


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_training_sort_permutations(pkg, dev, Nc, Nf, joint):
    c = _case(pkg, dev, Nc, Nf)
    d = c["d"]
    t_f = c["coarse"][2]
    chans = _channels(d["t_c"], t_f, d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"])
    out = c["merge", joint]
    _check_sort(pkg, chans, out, joint, Nc)
    bundle, w, C_f, perm, maps = out
    assert bool(torch.isfinite(bundle).all()) and bool(torch.isfinite(w).all()) and bool(torch.isfinite(C_f).all())
    # without maps: the same bits (k_merge<true> and k_merge_x<true, maps> end in one composite)
    b1, w1, C1, p1, _ = pkg.ops.merge_composite_train(d["t_c"], t_f, d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"], last=R.LAST, joint=bool(joint))
    assert torch.equal(_bits(b1), _bits(bundle)) and torch.equal(_bits(w1), _bits(w)) and torch.equal(_bits(C1), _bits(C_f)) and torch.equal(p1, perm)
    if not joint:  # the values-only sort of inference (k_merge<false>) gives the same bundle, weights and colour
        b0, w0, C0 = pkg.ops.merge_composite(d["t_c"], t_f, d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"], last=R.LAST)
        assert torch.equal(_bits(b0), _bits(bundle)) and torch.equal(_bits(w0), _bits(w)) and torch.equal(_bits(C0), _bits(C_f))


@pytest.mark.parametrize("joint", [0, 1])
def test_training_sort_on_exact_ties(pkg, dev, joint):
    t = _tie_case(pkg, dev)
    d = t["d"]
    chans = _channels(d["t_c"], d["t_f"], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"])
    _check_sort(pkg, chans, t["merge", joint], joint, 65)
    if not joint:
        b0, w0, C0 = pkg.ops.merge_composite(d["t_c"], d["t_f"], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"], last=R.LAST)
        bundle, w, C_f = t["merge", 0][:3]
        assert torch.equal(_bits(b0), _bits(bundle)) and torch.equal(_bits(w0), _bits(w)) and torch.equal(_bits(C0), _bits(C_f))


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", [(64, 65), (65, 63), (130, 200)])
def test_training_sort_on_adversarial_values(pkg, dev, Nc, Nf, joint):
    """the channels of test_merge_sort_network_on_adversarial_values -- negative numbers, both zeros, runs of duplicates, huge and tiny
    magnitudes, then NaNs of both signs -- through the entry that carries the original slots"""
    B, N = R.B_RAYS, Nc + Nf
    gen = torch.Generator().manual_seed(Nc)

    def channel():
        x = torch.randn(B, N, generator=gen) * torch.tensor([1e-30, 1.0, 1e30])[torch.randint(0, 3, (B, N), generator=gen)]
        x = torch.where(torch.rand(B, N, generator=gen) < 0.2, torch.round(x.clamp(-3, 3)), x)
        x = torch.where(torch.rand(B, N, generator=gen) < 0.05, -torch.zeros(B, N), x)
        return x

    ch = [channel() for _ in range(5)]
    nan_ch = [x.clone() for x in ch]
    for x in nan_ch:
        x[torch.rand(B, N, generator=gen) < 0.03] = float("nan")
        x[torch.rand(B, N, generator=gen) < 0.01] = -torch.tensor(float("nan"))
        x[:, N // 2] = float("nan")
    for name, (t, r, g, b, sg) in (("finite", ch), ("with NaNs", nan_ch)):
        chans = torch.stack((t, r, g, b, sg), dim=1)
        dd = lambda x: x.contiguous().to(dev)
        rgb = torch.stack((r, g, b), dim=2)
        out = pkg.ops.merge_composite_train(dd(t[:, :Nc]), dd(t[:, Nc:]), dd(sg[:, :Nc]), dd(sg[:, Nc:]), dd(rgb[:, :Nc]), dd(rgb[:, Nc:]),
                                            last=R.LAST, joint=bool(joint))
        _check_sort(pkg, chans, out, joint, Nc)
        if name == "with NaNs":
            assert bool(torch.isnan(chans).any(dim=2).all())  # every ray and channel holds a NaN: padding slots must stay behind them


# ---------------------------------------------------------------------------------------------------------------
# C. merged composite forward
# ---------------------------------------------------------------------------------------------------------------
def _merged_forward(label, out, exp_low):
    bundle, w, C_f, perm, maps = out
    b = bundle.cpu()
    with torch.no_grad():
        m64 = R.merged_composite(b[:, :, 0].double(), b[:, :, 1:4].double(), b[:, :, 4].double())
        m32 = R.merged_composite(b[:, :, 0], b[:, :, 1:4], b[:, :, 4])
        low = R.merged_composite(b[:, :, 0].double(), b[:, :, 1:4].double(), b[:, :, 4].double(), exp_low=exp_low)
    bars = Bars(label)
    for name, got in (("w", w), ("C_f", C_f), ("D_f", maps[:, 2]), ("A_f", maps[:, 3])):
        assert bool(torch.isfinite(got).all()), name
        bars.add(name, got.cpu(), m64[name], m32[name], low[name])
    assert bool(torch.isnan(maps[:, :2]).all())  # the coarse maps' columns are not this kernel's
    bars.check()


@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_merged_composite_forward_against_fp64(pkg, dev, Nc, Nf, joint):
    c = _case(pkg, dev, Nc, Nf)
    _merged_forward(f"C ({Nc}, {Nf}) joint={joint}", c["merge", joint], c["exp_low", joint])


def test_merged_composite_forward_on_exact_ties(pkg, dev):
    t = _tie_case(pkg, dev)
    _merged_forward("C ties (65, 63)", t["merge", 0], t["exp_low", 0])


# ---------------------------------------------------------------------------------------------------------------
# D. merge backward
# ---------------------------------------------------------------------------------------------------------------
NAMES_D = ("dsig_c", "dsig_f", "drgb_c", "drgb_f", "dt_f")


def _merge_backward(pkg, dev, label, out, exp_low, Nc, dC_f, dmaps):
    bundle, _, _, perm, _ = out
    got = pkg.ops.merge_composite_backward(bundle, perm, dC_f.to(dev), Nc, last=R.LAST, dmaps=None if dmaps is None else dmaps.to(dev))
    ref64 = R.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC_f, F64, dmaps)
    ref32 = R.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC_f, F32, dmaps)
    low = R.merged_grads(bundle.cpu(), perm.cpu(), Nc, dC_f, F64, dmaps, exp_low=exp_low)
    bars = Bars(label)
    for name, g, r64, r32, lo64 in zip(NAMES_D, got, ref64, ref32, low):
        assert bool(torch.isfinite(g).all()), (label, name, "an element was not written")  # (the outputs start as NaN)
        assert g.shape == r64.shape
        bars.add(name, g.cpu(), r64, r32, lo64)
    bars.check()
    if dmaps is not None:  # the maps alone: the colour branch receives exactly nothing
        z = pkg.ops.merge_composite_backward(bundle, perm, torch.zeros_like(dC_f).to(dev), Nc, last=R.LAST, dmaps=dmaps.to(dev))
        assert bool((z[2] == 0).all()) and bool((z[3] == 0).all())
        assert all(bool(torch.isfinite(q).all()) for q in z)


@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("joint", [0, 1])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_merge_backward_against_fp64(pkg, dev, Nc, Nf, joint, with_maps):
    c = _case(pkg, dev, Nc, Nf)
    _merge_backward(pkg, dev, f"D ({Nc}, {Nf}) joint={joint} maps={with_maps}", c["merge", joint], c["exp_low", joint], Nc, c["o"]["dC_f"],
                    c["o"]["dmaps"] if with_maps else None)


@pytest.mark.parametrize("with_maps", [False, True])
def test_merge_backward_on_exact_ties(pkg, dev, with_maps):
    t = _tie_case(pkg, dev)
    _merge_backward(pkg, dev, f"D ties (65, 63) maps={with_maps}", t["merge", 0], t["exp_low", 0], 65, t["o"]["dC_f"], t["o"]["dmaps"] if with_maps else None)


# ---------------------------------------------------------------------------------------------------------------
# E. coarse backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("Nc,Nf", SIZES)
def test_coarse_backward_against_fp64(pkg, dev, Nc, Nf, with_maps):
    c = _case(pkg, dev, Nc, Nf)
    o, d, rep = c["o"], c["d"], c["replica"]
    B = R.B_RAYS
    assert int(rep["ambiguous"].sum()) <= R.AMBIGUOUS_MAX * rep["ambiguous"].numel()
    dt_f = torch.where(rep["ambiguous"], torch.zeros_like(o["dt_f"]), o["dt_f"])  # zeroed BEFORE both sides run; nothing is excluded afterwards
    dmaps = o["dmaps"] if with_maps else None
    ref64 = R.coarse_grads(o, rep["k"], F64, dt_f, dmaps)
    ref32 = R.coarse_grads(o, rep["k"], F32, dt_f, dmaps)
    low = R.coarse_grads(o, rep["k"], F64, dt_f, dmaps, exp_low=c["exp_low"])
    # 8-ray buffers: rays 6, 7 are what the two waves behind the batch would touch if they stored anything
    pad = lambda x: torch.cat((x, x[:2]), 0).to(dev).contiguous()
    args = (pad(o["t_c"]), pad(o["sig_c"]), pad(o["rgb_c"]), torch.cat((o["near"], o["near"][:2])), torch.cat((o["far"], o["far"][:2])), o["delta0"],
            pad(o["dC_c"]), pad(dt_f))
    dm = None if dmaps is None else pad(dmaps)
    SENTINEL = 123.0

    def run(rays, calls=1):
        dsig, drgb = torch.zeros(B + 2, Nc, device=dev), torch.zeros(B + 2, Nc, 3, device=dev)
        dsig[rays:] = SENTINEL
        drgb[rays:] = SENTINEL
        for _ in range(calls):
            pkg.ops.coarse_composite_backward_add(*args, dsig, drgb, dmaps=dm, rays=rays)
        assert bool((dsig[rays:] == SENTINEL).all()) and bool((drgb[rays:] == SENTINEL).all()), f"{rays}-ray call stored behind its batch"
        return dsig[:rays], drgb[:rays]

    dsig, drgb = run(B)
    assert bool(torch.isfinite(dsig).all()) and bool(torch.isfinite(drgb).all())
    bars = Bars(f"E ({Nc}, {Nf}) maps={with_maps}")
    bars.add("dsig_c", dsig.cpu(), ref64[0], ref32[0], low[0])
    bars.add("drgb_c", drgb.cpu(), ref64[1], ref32[1], low[1])
    # "ADDS": a second call into the same buffers doubles them (g + g is exact)
    dsig2, drgb2 = run(B, calls=2)
    assert torch.equal(_bits(dsig2), _bits(2 * dsig)) and torch.equal(_bits(drgb2), _bits(2 * drgb))
    # a 4-ray call (one full workgroup): the same bits for its rays
    dsig4, drgb4 = run(4)
    assert torch.equal(_bits(dsig4), _bits(dsig[:4])) and torch.equal(_bits(drgb4), _bits(drgb[:4]))
    if not with_maps:  # the entry without dmaps is the same launch
        a, b = pkg.ops.coarse_composite_backward(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], d["dC_c"], dt_f.to(dev))
        assert torch.equal(_bits(a), _bits(dsig)) and torch.equal(_bits(b), _bits(drgb))
    bars.check()
