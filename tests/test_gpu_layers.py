"""GPU: every forward layer and every layer of the dX chain against a float64 evaluation of its own saved operands.

tests/test_gpu_weight_gradients.py holds the weight-gradient products to their operands, but takes those operands as given: the saved
layer inputs and the chain's pre-activation gradients go into the device gradient and into its reference alike.  Here each of them is
checked in turn, one layer at a time, from the device's own input of that layer (tests/ws_operands.py: iter_layer_reference,
iter_chain_reference), so the sort and ReLU discontinuities of the whole step do not arise.  Bars, fixed from
the error model before any run (E = element bar of one accumulation, relative to that element's magnitude |W| |x| + |b|):
  fp32, fp32_tile   |dev - ref| <= E mag, E = 2^-20 (the k-ordered fp32 MFMA chain: measured 0.75-1.5e-7 of sum |ab| for K <= 1024);
                    2 E mag for the two layers behind the point_info fold (forward c, chain g7: two accumulations, _stages)
  bf16              dev inside [R(f(ref - E mag)), R(f(ref + E mag))], E = 2^-18, R = exact RNE to bf16, f = ReLU where the layer has one
  split             |hi + mid - ref| <= E mag + 2^-17 |ref|, E = 2^-18; hi == R(hi + mid) and |mid| <= ulp_bf16(hi) / 2, except that
                    where mid's own rounding reached |mid| == ulp / 2 exactly the pair is a tie R resolves to even (counted, printed)
  masks             a bit equals ref_pre > 0 wherever |ref_pre| > E mag (inside that band either value is accepted; counted)
  dz, dspre         bit for bit the fp32 expressions of field_bwd_reg.hip:233-246 (bf16 / split: their RNE parts)
  rgb               |rgb - sigmoid(z_ref)| <= sigmoid'(z_ref) E mag_z + 2^-21 sigmoid(z_ref) (expf, add, divide: a few fp32 ulp)
Every mode writes drgb_* / dsig_* to its workspace (the fused small-batch bf16 stages too), so every chain check starts there.
"""
import pytest
import torch

import ws_operands as W

pytestmark = pytest.mark.gpu

E_FP32 = 2.0 ** -20
E_BF16 = 2.0 ** -18
SPLIT_REL = 2.0 ** -17   # hi + mid represents the fp32 value to about 2^-17 of itself
RGB_REL = 2.0 ** -21
TEETH = 4.0

ARITHS = ("fp32", "fp32_tile", "bf16_mlp", "split_train")
MODE = {"fp32": "fp32", "fp32_tile": "fp32", "bf16_mlp": "bf16", "split_train": "split"}
SIZES = [(2, 2, 1), (50, 24, 40), (130, 31, 65), (853, 64, 128), (3, 1024, 1024), (4096, 64, 128)]
AUTOGRAD_SIZE = (130, 31, 65)
CASES = [pytest.param(a, *s, "train_step", id=f"{a}-{s[0]}x{s[1]}+{s[2]}-train_step") for a in ARITHS for s in SIZES] + \
        [pytest.param(a, *AUTOGRAD_SIZE, "autograd", id=f"{a}-{AUTOGRAD_SIZE[0]}x{AUTOGRAD_SIZE[1]}+{AUTOGRAD_SIZE[2]}-autograd")
         for a in ARITHS]


def _flags(arith):
    from nerf_tiny_amd import _abi

    return _abi.SAVE_FOR_BACKWARD | {"fp32": 0, "fp32_tile": _abi.FORCE_TILE_KERNEL, "bf16_mlp": _abi.BF16_MLP,
                                     "split_train": _abi.SPLIT_MLP}[arith]


def _model(pkg, w, arith, B, Nc, Nf, dev):
    m = pkg.NeRFModel(Nc, Nf, B)
    m.load_state_dict(w)
    m = m.to(dev)
    m.force_tile_kernel = arith == "fp32_tile"
    m.bf16_mlp = arith == "bf16_mlp"
    m.split_train = arith == "split_train"
    return m


def _inputs(oracle, B, Nc, Nf):
    return oracle.lego_inputs(B, seed=5) if (Nc, Nf) == (64, 128) else oracle.fern_inputs(B, seed=9)


def _step(m, entry, inputs, dev):
    row, col, pb, K, Ct = inputs
    if entry == "train_step":
        m.train_step(row, col, pb, K, Ct)
    else:
        Cc, Cf = m(row, col, pb, K)
        m.ray_loss(Cc, Cf, Ct.to(dev)).backward()


# ---- the statistics: ratio of each element's error to its bar (<= 1 passes) -----------------------------------------------------
def _over(err, bar):
    """err / bar, where bar == 0 demands err == 0."""
    return torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))


def _bf16_preimage(d, relu, rnd="rne"):
    """[lo, hi]: the accumulator values that round (rnd) to the bf16 value d -- after a ReLU (relu) 0 is every value <= 0."""
    a = d.abs()
    u = W.ulp_bf16(a)
    if rnd == "rne":
        frac, _ = torch.frexp(a)
        down = torch.where(frac == 0.5, u / 4, u / 2)  # below a power of two the spacing halves
        up = u / 2
    else:  # truncation toward zero: |acc| in [|d|, |d| + ulp)
        down, up = torch.zeros_like(u), u
    lo = torch.where(d < 0, d - up, d - down)
    hi = torch.where(d < 0, d + down, d + up)
    zero = d == 0
    tiny = 2.0 ** (W.BF16_EMIN - 1)
    lo = torch.where(zero, torch.full_like(d, -float("inf") if relu else -tiny), lo)
    hi = torch.where(zero, torch.full_like(d, tiny), hi)
    return lo, hi


def ratio(mode, dev_parts, ref, mag, relu, rnd="rne"):
    """Per element: the error over the bar of mode (fp32 / bf16 / split).  bf16: the distance from ref to the accumulator values that
    round to the device's bf16 result, over E mag."""
    if mode == "fp32":
        return _over((dev_parts[0].double() - ref).abs(), E_FP32 * mag)
    if mode == "bf16":
        lo, hi = _bf16_preimage(dev_parts[0].double(), relu, rnd)
        return _over((lo - ref).clamp_min(0) + (ref - hi).clamp_min(0), E_BF16 * mag)
    return _over((dev_parts[0].double() + dev_parts[1].double() - ref).abs(), E_BF16 * mag + SPLIT_REL * ref.abs())


def bf16_interval_ok(dev, ref, mag, relu, E=E_BF16, rnd=W.rne_bf16):
    """dev inside [R(f(ref - E mag)), R(f(ref + E mag))]: R and ReLU are monotone, so this is every result an fp32 accumulation within
    E mag of ref rounds to."""
    f = (lambda x: x.clamp_min(0)) if relu else (lambda x: x)
    d = dev.double()
    return (d >= rnd(f(ref - E * mag))) & (d <= rnd(f(ref + E * mag)))


def split_structure(hi, mid):
    """(violations, ties): hi == R(hi + mid) and |mid| <= ulp(hi) / 2 must hold, except that |mid| == ulp(hi) / 2 exactly may round
    either way (mid = RNE(x - hi) can round up to the half ulp when hi is odd; then R(hi + mid) is hi's even neighbour)."""
    h, md = hi.double(), mid.double()
    half = W.ulp_bf16(h) / 2
    tie = (md.abs() == half) & (h != 0)
    bad = (md.abs() > half) | ((W.rne_bf16(h + md) != h) & ~tie) | ((h == 0) & (md != 0))
    return int(bad.sum()), int(tie.sum())


def _stages(mode, name):
    """Accumulations behind one element of a layer, each within E of its own magnitude.  fp32 runs point_info and dir_info's feature
    columns (forward c, chain g7) as two: the register kernels through a W_fold formed per call by fp32 fma chains (its rounding bounded
    by E |W_dir[:, 24:]| |W_pi|), the tile kernels as two products in sequence; either way the second stage's magnitude is at most the
    fold's, so the bar of those layers is 2 E mag.  bf16 / split multiply by the device's own W_fold: one accumulation."""
    return 2 if mode == "fp32" and name in ("c", "g7") else 1


class Worst:
    """The worst ratio over a case, with the tensor, pass and row it came from."""

    def __init__(self, n_coarse):
        self.n_coarse, self.value, self.where = n_coarse, 0.0, "-"

    def add(self, name, r):
        flat = r.reshape(r.shape[0], -1).amax(1) if r.dim() > 1 else r
        i = int(flat.argmax())
        v = float(flat[i])
        if v > self.value or self.where == "-":
            p, row = ("coarse", i) if i < self.n_coarse else ("fine", i - self.n_coarse)
            self.value, self.where = v, f"{name} {p} row {row}"
        return v


def _check_forward(ops, weights, mode, worst, per):
    band = 0
    E = E_FP32 if mode == "fp32" else E_BF16
    for name, (ref, mag, pre) in W.iter_layer_reference(ops, weights, mode):
        mag = _stages(mode, name) * mag
        if name == "sigma":
            assert torch.equal(ops["sig"][0], ops["spre"][0].abs()), "sigma is not |spre|"
            continue
        if name == "rgb":
            s = torch.sigmoid(pre)
            r = _over((ops["rgb"][0].double() - ref).abs(), s * (1 - s) * E * mag + RGB_REL * s)
            per[name] = worst.add(name, r)
            assert per[name] <= 1.0, (name, per[name], worst.where)
            continue
        relu = name != "spre"
        dev = ops[name] if relu else ops["spre"]
        # spre is the fp32 accumulator in every mode
        r = ratio(mode, dev, ref, mag, relu) if relu else _over((dev[0].double() - ref).abs(), E * mag)
        per[name] = worst.add(name, r)
        if mode == "bf16" and relu:
            ok = bf16_interval_ok(dev[0], ref, mag, relu)
            assert bool(ok.all()), (name, int((~ok).sum()))
        if mode == "split" and relu:
            bad, ties = split_structure(*dev)
            assert bad == 0, (name, bad)
            per[name + " ties"] = ties
        assert per[name] <= 1.0, (name, per[name], worst.where)
        if relu:
            mk = ops["mc" if name == "c" else "m" + name[1:]][0][:, :ref.shape[1]]
            clear = pre.abs() > E * mag
            wrong = clear & (mk != (pre > 0))
            assert not bool(wrong.any()), (name, "mask", int(wrong.sum()))
            band += int((~clear).sum())
        del ref, mag, pre
    return band


def _check_upstream(ops, mode):
    dz, ds = W.upstream_reference(ops)
    if mode == "fp32":
        assert torch.equal(ops["dz"][0], dz) and torch.equal(ops["dspre"][0][:, 0], ds)
        return
    want = (dz, ds[:, None])
    for got, v in zip((ops["dz"], ops["dspre"]), want):
        v = v.double()
        hi = W.rne_bf16(v)
        assert torch.equal(got[0].double(), hi)
        if mode == "split":
            assert torch.equal(got[1].double(), W.rne_bf16(v - hi))


def _check_chain(ops, weights, mode, worst, per):
    for name, (ref, mag) in W.iter_chain_reference(ops, weights, mode):
        mag = _stages(mode, name) * mag
        r = ratio(mode, ops[name], ref, mag, relu=False)
        per[name] = worst.add(name, r)
        if mode == "bf16":
            ok = bf16_interval_ok(ops[name][0], ref, mag, relu=False)
            assert bool(ok.all()), (name, int((~ok).sum()))
        if mode == "split":
            bad, ties = split_structure(*ops[name])
            assert bad == 0, (name, bad)
        assert per[name] <= 1.0, (name, per[name], worst.where)
        del ref, mag


def _teeth(ops, weights, mode, B, Nc, Nf):
    """Perturb the REFERENCE (never the device data) over the last, possibly ragged, wave block of the fine pass and recompute the
    same statistic: each perturbation must move it to at least TEETH x its bar."""
    a = B * Nc + ((B * Nf - 1) // W.WAVE_ROWS) * W.WAVE_ROWS
    b = B * (Nc + Nf)
    blk = W.rows(ops, a, b)
    out = {}
    # one 8-feature k-block of layer 5's input dropped
    x = blk["h4"][0]
    kb = next((k for k in range(W.WIDTH // 8) if bool((x[:, 8 * k:8 * k + 8] != 0).any())), 0)
    drop = dict(blk)
    drop["h4"] = tuple(t.clone().index_fill_(1, torch.arange(8 * kb, 8 * kb + 8, device=t.device), 0) for t in blk["h4"])
    ref, mag, _ = W.layer_reference(drop, weights, mode)["h5"]
    out["k-block"] = float(ratio(mode, blk["h5"], ref, mag, True).max())
    # one mask bit flipped where the layer is far from its kink and the gradient it gates is non-zero
    ch = W.chain_reference(blk, weights, mode)
    ref6, mag6 = ch["g6"]
    pre6 = W.layer_reference(blk, weights, mode)["h6"][2]
    E = E_FP32 if mode == "fp32" else E_BF16
    score = torch.where(blk["m6"][0] & (pre6.abs() > 1e3 * E * W.layer_reference(blk, weights, mode)["h6"][1]), ref6.abs(), 0)
    i = int(score.argmax())
    flip = dict(blk)
    m6 = blk["m6"][0].clone()
    m6.view(-1)[i] = ~m6.view(-1)[i]
    flip["m6"] = (m6,)
    ref, mag = W.chain_reference(flip, weights, mode)["g6"]
    out["mask bit"] = float(ratio(mode, blk["g6"], ref, mag, False).max())
    if mode == "bf16":
        ref, mag, _ = W.layer_reference(blk, weights, mode)["h5"]
        out["truncation"] = float(ratio(mode, blk["h5"], ref, mag, True, rnd="trunc").max())
    if mode == "split":
        ref, mag, _ = dict(W.iter_layer_reference(blk, weights, mode, terms=((0, 0), (0, 1))))["h5"]
        out["no mid.hi"] = float(ratio(mode, blk["h5"], ref, mag, True).max())
    return out


@pytest.mark.parametrize("arith,B,Nc,Nf,entry", CASES)
def test_layers_against_fp64_of_their_own_operands(oracle, pkg, dev, arith, B, Nc, Nf, entry):
    inputs = _inputs(oracle, B, Nc, Nf)
    m = _model(pkg, oracle.make_weights(6, sharp=True), arith, B, Nc, Nf, dev)
    _step(m, entry, inputs, dev)
    mode = MODE[arith]
    ops = W.read_layer_operands(m.last_workspace, B, Nc, Nf, _flags(arith))
    weights = [p.detach() for p in m.network.parameters()]
    fwd, chn = Worst(B * Nc), Worst(B * Nc)
    per = {}
    band = _check_forward(ops, weights, mode, fwd, per)
    _check_upstream(ops, mode)
    _check_chain(ops, weights, mode, chn, per)
    teeth = _teeth(ops, weights, mode, B, Nc, Nf)
    ties = sum(v for k, v in per.items() if k.endswith("ties"))
    print(f"\n{arith} {B}x({Nc}+{Nf}) {entry}: forward worst {fwd.value:.3f} x bar ({fwd.where}); chain worst {chn.value:.3f} x bar "
          f"({chn.where}); mask entries inside the band {band}" + (f"; split tie pairs {ties}" if mode == "split" else "") +
          "; teeth " + ", ".join(f"{k} {v:.3g} x bar" for k, v in teeth.items()))
    for k, v in teeth.items():
        assert v >= TEETH, (k, v)


# ---- the inference forward and the saving forward: the same bits -----------------------------------------------------------------
@pytest.mark.parametrize("arith,B,Nc,Nf", [("fp32", 4096, 64, 128), ("fp32", 130, 31, 65), ("split", 4096, 64, 128),
                                           ("split", 130, 31, 65)])
def test_inference_and_saving_forward_give_the_same_bits(oracle, pkg, dev, arith, B, Nc, Nf):
    """k_field_fwd_reg<SAVE=false> and <SAVE=true> share one template and its source arithmetic (the library is built with
    -ffp-contract=off), and so do the split kernel's two forms (launch_field_fwd_split(f, save)): per-sample outputs, fine depths and
    both colours are bit-equal.  split: split_mlp's inference against split_train's forward."""
    from nerf_tiny_amd import _abi

    row, col, pb, K, _ = _inputs(oracle, B, Nc, Nf)
    m = _model(pkg, oracle.make_weights(8, sharp=True), "fp32", B, Nc, Nf, dev)
    m.split_mlp = m.split_train = arith == "split"
    flags = _abi.SPLIT_MLP if arith == "split" else 0
    names = [("sig_c", (B * Nc,)), ("rgb_c", (B * Nc, 3)), ("t_f", (B * Nf,)), ("sig_f", (B * Nf,)), ("rgb_f", (B * Nf, 3))]
    with torch.no_grad():
        Ci = [c.clone() for c in m(row, col, pb, K)]
    ws = m._ws[flags][1]
    inf = [_abi.ws_view(ws, B, Nc, Nf, flags, n, s).clone() for n, s in names]
    Ct = m(row, col, pb, K)
    ws = m.last_workspace
    tr = [_abi.ws_view(ws, B, Nc, Nf, flags | _abi.SAVE_FOR_BACKWARD, n, s) for n, s in names]
    for (n, _), a, b in zip(names, inf, tr):
        assert torch.equal(a, b), n
    assert torch.equal(Ci[0], Ct[0].detach()) and torch.equal(Ci[1], Ct[1].detach())


# ---- dead units: an all-zero weight row and a zero bias ----------------------------------------------------------------------------
DEAD = [17 + 29 * l for l in range(8)]  # one unit of each of point_layer.0..7
DEAD_DIR = 77                           # and one of dir_info


@pytest.mark.parametrize("arith", ARITHS)
def test_dead_units_stay_dead(oracle, pkg, dev, arith):
    """A unit whose pre-activation is exactly +0 for every sample (0 . x + 0) is dead, as torch's ReLU backward and oracle.loss_and_grads
    have it: its weight and bias gradients are exactly 0, its saved activations are 0, and so are its mask bits."""
    B, Nc, Nf = 130, 31, 65
    w = oracle.make_weights(6, sharp=True)
    for l, u in enumerate(DEAD):
        w[f"network.point_layer.{l}.0.weight"][u] = 0
        w[f"network.point_layer.{l}.0.bias"][u] = 0
    w["network.dir_info.0.weight"][DEAD_DIR] = 0
    w["network.dir_info.0.bias"][DEAD_DIR] = 0
    m = _model(pkg, w, arith, B, Nc, Nf, dev)
    _step(m, "train_step", _inputs(oracle, B, Nc, Nf), dev)
    g = [p.grad for p in m.network.parameters()]
    ops = W.read_layer_operands(m.last_workspace, B, Nc, Nf, _flags(arith))
    for l, u in enumerate(DEAD):
        assert int((g[2 * l][u] != 0).sum()) == 0 and float(g[2 * l + 1][u]) == 0, (arith, f"point_layer.{l} gradient")
        assert all(bool((t[:, u] == 0).all()) for t in ops[f"h{l}"]), (arith, f"h{l} saved")
        assert not bool(ops[f"m{l}"][0][:, u].any()), (arith, f"h{l} mask", int(ops[f"m{l}"][0][:, u].sum()))
    assert int((g[W.W_DIR][DEAD_DIR] != 0).sum()) == 0 and float(g[W.B_DIR][DEAD_DIR]) == 0, (arith, "dir_info gradient")
    assert all(bool((t[:, DEAD_DIR] == 0).all()) for t in ops["c"]), (arith, "c saved")
    assert not bool(ops["mc"][0][:, DEAD_DIR].any()), (arith, "c mask")
