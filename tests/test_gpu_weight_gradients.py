"""GPU: every weight-gradient schedule against a float64 evaluation of its own operands.

The whole-step gradient tests have to be loose (the reference's own gradient is ill-conditioned).  The
weight-gradient products are not: after a backward the workspace still holds exactly what they read (tests/ws_operands.py), so
the same products evaluated in float64 leave only the kernels' fp32 accumulation order as a difference.  Every one of the 24
gradient tensors is held to ||dW - ref|| / ||mag|| < BAR, mag being the same formula on absolute values.

The matrix reaches every schedule csrc/api.hip's backward_impl (fp32) and csrc/dw_bf16.hip's launch_dw_bf16_phase (bf16, split) choose
between (expected_path below restates the choice):
  fp32         ray duty on / off: the dir_info product writes the per-ray sums itself (dw_ray_duty_ok) or launch_small_grads does
  bf16, split  (a) <= 5120 wave blocks, no early event: one k_dw_bf16_multi launch
               (b) <= 5120, event: two multi launches, early then late
               (c) >  5120, no event: one k_dw_bf16 launch for the group of six products, a multi launch for four
               (d) >  5120, event: a launch per product
on both sides of the switch (852 / 853 rays), with ragged last wave blocks in both passes, and at both size limits.  Every case
with the event also checks its promise (include/nerf_hip.h: tensors 0..15 are final when it fires).
"""
import pytest
import torch

import ws_operands as W
from test_gpu_backward import GTOL, NOISE_BAND, _oracle_with_grads, _train_step
from conftest import l2_rel

pytestmark = pytest.mark.gpu

BAR = 1e-6    # fp32 accumulation over up to 786k rows, relative to the magnitude
TEETH = 4.0   # one wave block dropped from or doubled in the reference moves the statistic at least this far above BAR

# ---- which schedule a case selects (restated from the library) ---------------------------------------------------------------
DW_BF16_MULTI_MAX_WB = 5120  # csrc/dw_bf16.hip DW_BF16_MULTI_MAX_WB
DW4_DEPTH = 8                # csrc/dw_f32.hip:139
DW_WGS = 256                 # csrc/kernels.h:227: workgroups of the dir_info product (not one of the grouped seven)
DIR_MSUBS = 2                # csrc/dw_f32.hip:314-318: nout 128, nin 256 -> 4 waves over 2 blocks


def dw_ray_duty_ok(B, Nc, Nf):
    """csrc/dw_f32.hip:660-666 for the dir_info product."""
    if Nc % (2 * DW4_DEPTH) or Nf % (2 * DW4_DEPTH):
        return False
    rows = B * (Nc + Nf)
    gran = 2 * DW4_DEPTH * DIR_MSUBS
    per_wg = (-(-rows // DW_WGS) + gran - 1) // gran * gran
    per_wave = per_wg // DIR_MSUBS
    return per_wave % Nc == 0 and per_wave % Nf == 0 and (B * Nc) % Nf == 0 and rows % per_wave == 0


def expected_path(arith, B, Nc, Nf, event):
    if arith == "fp32":
        return "duty" if dw_ray_duty_ok(B, Nc, Nf) else "noduty"
    wb_tot = W.wave_blocks(B, Nc) + W.wave_blocks(B, Nf)  # csrc/api.hip wave_blocks(), backward_impl()
    small = wb_tot <= DW_BF16_MULTI_MAX_WB                  # csrc/dw_bf16.hip dw_bf16_multi(), launch_dw_bf16_phase()
    return ("b" if event else "a") if small else ("d" if event else "c")


ARITHS = ("fp32", "bf16_mlp", "split_train")
SIZES = [(2, 2, 1), (50, 24, 40), (400, 64, 128), (852, 64, 128), (853, 64, 128), (1024, 64, 128), (3, 1024, 1024), (4096, 64, 128)]
# the autograd forward + backward() route (nerf_hip_backward_overlap) instead of model.train_step: at 400 rays it differs (the train
# step fuses ray_loss into the fine pass's epilogue; bf16 runs the per-ray stages inside the field and chain launches either way)
AUTOGRAD = {(2, 2, 1, False), (400, 64, 128, False), (853, 64, 128, True)}


def _cases():
    out = []
    for arith in ARITHS:
        for B, Nc, Nf in SIZES:
            for event in (False, True):
                if event and B == 4096:
                    continue
                entry = "autograd" if (B, Nc, Nf, event) in AUTOGRAD else "train_step"
                path = expected_path(arith, B, Nc, Nf, event)
                out.append(pytest.param(arith, B, Nc, Nf, event, entry,
                                        id=f"{arith}-{B}x{Nc}+{Nf}-{'event' if event else 'noevent'}-{entry}-{path}"))
    return out


CASES = _cases()
_reached = {(c.values[0], expected_path(*c.values[:5])) for c in CASES}
assert all((a, p) in _reached for a in ("bf16_mlp", "split_train") for p in "abcd"), _reached
assert {("fp32", "duty"), ("fp32", "noduty")} <= _reached, _reached
assert {e for *_, e in (c.values for c in CASES)} == {"train_step", "autograd"}
assert {c.values[0] for c in CASES if c.values[5] == "autograd"} == set(ARITHS)


def _inputs(oracle, B, Nc, Nf):
    return oracle.lego_inputs(B, seed=5) if (Nc, Nf) == (64, 128) else oracle.fern_inputs(B, seed=9)


def _model(pkg, oracle, arith, B, Nc, Nf, dev):
    m = pkg.NeRFModel(Nc, Nf, B)
    m.load_state_dict(oracle.make_weights(6, sharp=True))
    m = m.to(dev)
    m.bf16_mlp = arith == "bf16_mlp"
    m.split_train = arith == "split_train"
    return m


def _flags(arith):
    from nerf_tiny_amd import _abi

    return _abi.SAVE_FOR_BACKWARD | {"fp32": 0, "bf16_mlp": _abi.BF16_MLP, "split_train": _abi.SPLIT_MLP}[arith]


def _step(m, entry, inputs, dev):
    row, col, pb, K, Ct = inputs
    if entry == "train_step":
        m.train_step(row, col, pb, K, Ct)
    else:
        Cc, Cf = m(row, col, pb, K)
        m.ray_loss(Cc, Cf, Ct.to(dev)).backward()


def _step_with_early_copy(m, entry, inputs, dev):
    """One step with an overlap bucket; a side stream behind bucket.early_event copies tensors 0..15 as soon as the event fires.
    Returns (the copies, the final views).  The views start as NaN, so a copy taken before the early products were reduced differs."""
    from nerf_tiny_amd import parallel

    bucket = parallel.GradBucket(m.network.parameters()).enable_overlap()
    m.grad_bucket = bucket
    early = bucket.views[:parallel.EARLY_TENSORS]
    for v in early:
        v.fill_(float("nan"))
    _step(m, entry, inputs, dev)
    side = torch.cuda.Stream(dev)
    side.wait_event(bucket.early_event)
    with torch.cuda.stream(side):
        copies = [v.clone() for v in early]
    torch.cuda.synchronize(dev)
    bucket.consume()
    return copies, early


def _drop_range(B, Nc, Nf):
    """Real rows of one full wave block in the middle of the fine pass (one row where that pass has no full block)."""
    full = B * Nf // W.WAVE_ROWS
    if full == 0:
        return B * Nc + B * Nf // 2, 1
    return B * Nc + (full // 2) * W.WAVE_ROWS, W.WAVE_ROWS


@pytest.mark.parametrize("arith,B,Nc,Nf,event,entry", CASES)
def test_weight_gradients_against_fp64_products_of_their_operands(oracle, pkg, dev, arith, B, Nc, Nf, event, entry):
    inputs = _inputs(oracle, B, Nc, Nf)
    m = _model(pkg, oracle, arith, B, Nc, Nf, dev)
    if event:
        copies, early = _step_with_early_copy(m, entry, inputs, dev)
        for i, (c, v) in enumerate(zip(copies, early)):
            assert torch.equal(c, v), f"tensor {i} changed after early_event fired"
    else:
        _step(m, entry, inputs, dev)
    params = list(m.network.parameters())
    grads = [p.grad for p in params]
    assert all(torch.isfinite(g).all() for g in grads)
    ops = W.read_operands(m.last_workspace, B, Nc, Nf, _flags(arith))
    weights = [p.detach() for p in params]
    ref = W.dw_reference(ops, weights)
    stats = [W.dw_statistic(g, r, mag) for g, (r, mag) in zip(grads, ref)]
    # the bar has teeth: the reference without, or with twice, one wave block's rows puts the case far outside it.  (Per tensor the
    # margin is thinner where the block's share of the magnitude is small -- the sigma-head bias at 4096 rays moves < BAR: printed.)
    lo, n = _drop_range(B, Nc, Nf)
    delta = W.dw_reference(W.rows(ops, lo, lo + n), weights)
    drop = [W.dw_statistic(g, r - d, mag) for g, (r, mag), (d, _) in zip(grads, ref, delta)]
    double = [W.dw_statistic(g, r + d, mag) for g, (r, mag), (d, _) in zip(grads, ref, delta)]
    names = [k for k, _ in m.network.named_parameters()]
    worst = max(range(24), key=lambda i: stats[i])
    weakest = min(range(24), key=lambda i: min(drop[i], double[i]))
    teeth = min(max(drop), max(double))
    print(f"\n{arith} {B}x({Nc}+{Nf}) event={event} {entry} path={expected_path(arith, B, Nc, Nf, event)}: worst {stats[worst]:.2e} "
          f"({names[worst]}); one block dropped / doubled: {max(drop):.2e} / {max(double):.2e} = {teeth / BAR:.0f} x BAR "
          f"(weakest tensor {names[weakest]} {min(drop[weakest], double[weakest]) / BAR:.2g} x BAR)")
    for i in range(24):
        assert stats[i] < BAR, (names[i], stats[i])
    assert teeth > TEETH * BAR, (max(drop), max(double))


@pytest.mark.parametrize("B", [1024, 4096])
def test_fp32_gradients_have_the_same_bits_with_and_without_the_early_event(oracle, pkg, dev, B):
    """The two launch ranges of the early-event schedule give every product the same workgroup split as the one launch."""
    inputs = _inputs(oracle, B, 64, 128)
    m = _model(pkg, oracle, "fp32", B, 64, 128, dev)
    _step(m, "train_step", inputs, dev)
    plain = [p.grad.clone() for p in m.network.parameters()]
    copies, _ = _step_with_early_copy(m, "train_step", inputs, dev)
    for i, (a, p) in enumerate(zip(plain, m.network.parameters())):
        assert torch.equal(a, p.grad), i
    for i, c in enumerate(copies):
        assert torch.equal(c, plain[i]), i


@pytest.mark.parametrize("B,Nc,Nf", [(2, 2, 1), (3, 1024, 1024)])
def test_exact_backward_at_the_size_limits_against_the_oracle(oracle, pkg, dev, B, Nc, Nf):
    """The smallest batch and the most samples per ray, in the form of test_gpu_backward.py::test_odd_sizes_coarse_only: the coarse-only
    loss within GTOL; the full loss with the oracle's sort order and ReLU masks replayed (at 1024 + 1024 the merge backward sorts 2048
    samples) within NOISE_BAND."""
    inputs = oracle.fern_inputs(B, seed=9)
    w = oracle.make_weights(6, sharp=True)
    p, st, oloss = _oracle_with_grads(oracle, w, inputs, Nc, Nf, coarse_only=True)
    m, loss = _train_step(pkg, oracle, dev, w, inputs, Nc, Nf, coarse_only=True)
    assert abs(float(loss) - float(oloss)) <= 1e-5 * float(oloss)
    for (k, ref), q in zip(p.items(), m.network.parameters()):
        assert l2_rel(q.grad, ref.grad) < GTOL, k
    p, st, oloss = _oracle_with_grads(oracle, w, inputs, Nc, Nf)
    std = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in st.items()}
    m, loss = _train_step(pkg, oracle, dev, w, inputs, Nc, Nf, ref_stages=std)
    assert abs(float(loss) - float(oloss)) <= 1e-5 * float(oloss)
    for (k, ref), q in zip(p.items(), m.network.parameters()):
        assert l2_rel(q.grad, ref.grad) < NOISE_BAND, k
