"""CPU: tests/ray_stage_reference.py pinned to the oracle, and the conditions tests/test_gpu_ray_stages.py relies on.

  * the reference's graphs, run in float32 with the oracle's bins / sort order, give what the oracle's own weights_from_sigma / resample /
    composite autograd gives on the stages of two goldens (the same formulas op for op: bar 1e-6, about 16 fp32 ulps, for values and 1e-5 for
    the gradients, whose sums autograd may add up in another order);
  * the decision replica's bins are the oracle's on those goldens;
  * every case's seeded operands leave at most 1 % of the fine samples ambiguous (on the replica's own fp32 weights);
  * stable_order is the order it says it is;
  * the stage entry points the GPU file calls are declared in the header and bound in _abi.EXPORTS.
"""
import math
import os
import re

import pytest
import torch

from conftest import ROOT, golden_inputs, load_golden
import ray_stage_reference as R

GOLDENS = ["small_16_32", "cfg1_lego_crop32"]
NEW_EXPORTS = ("nerf_hip_coarse_composite_maps", "nerf_hip_coarse_composite_backward_maps", "nerf_hip_merge_composite_train",
               "nerf_hip_merge_composite_backward")


@pytest.fixture(scope="module", params=GOLDENS)
def stages(request, oracle):
    g = load_golden(request.param)
    row, col, pb, K, _ = golden_inputs(g)
    Nc, Nf = int(g["Nc"]), int(g["Nf"])
    st = {}
    with torch.no_grad():
        oracle.render(oracle.make_weights(int(g["seed"]), bool(g["sharp"])), row, col, pb, K, Nc, Nf, stages=st)
    st = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in st.items()}
    st["Nc"], st["Nf"] = Nc, Nf
    return st


def test_coarse_reference_is_the_oracles_graph(oracle, stages):
    st, Nc, Nf = stages, stages["Nc"], stages["Nf"]
    B = st["t_c"].shape[0]
    gen = torch.Generator().manual_seed(3)
    o = dict(Nc=Nc, Nf=Nf, near=st["near"], far=st["far"], t_c=st["t_c"], delta0=float(st["t_c"][0, 1] - st["t_c"][0, 0]),
             sig_c=st["sig_c"], rgb_c=st["rgb_c"], dC_c=torch.randn(B, 3, generator=gen))
    g_t = torch.randn(B, Nf, generator=gen) * 0.01
    g_m = torch.randn(B, 4, generator=gen)
    # the oracle's own autograd of the same loss
    sig = st["sig_c"].clone().requires_grad_(True)
    rgb = st["rgb_c"].clone().requires_grad_(True)
    w_c = oracle.weights_from_sigma(((st["far"] - st["near"]) / Nc)[:, None].expand(-1, Nc), sig)
    t_f, rs = oracle.resample(st["t_c"], w_c, Nf)
    C_c = oracle.composite(w_c, rgb)
    D_c, A_c = (w_c * st["t_c"]).sum(1), w_c.sum(1)
    ((t_f * g_t).sum() + (C_c * o["dC_c"]).sum() + (D_c * g_m[:, 0]).sum() + (A_c * g_m[:, 1]).sum()).backward()
    assert torch.equal(rs["k"], st["k"])
    with torch.no_grad():
        s = R.coarse_stage(st["sig_c"], st["rgb_c"], st["t_c"], st["near"], st["far"], o["delta0"], Nf, st["k"])
    assert s["w"].dtype == torch.float32
    errs = {n: R.l2_rel(s[n], ref.detach()) for n, ref in (("w", w_c), ("cdf", rs["cdf"]), ("t_f", t_f), ("C_c", C_c), ("D_c", D_c), ("A_c", A_c))}
    dsig, drgb = R.coarse_grads(o, st["k"], torch.float32, g_t, g_m)
    gerrs = dict(dsig=R.l2_rel(dsig, sig.grad), drgb=R.l2_rel(drgb, rgb.grad))
    print({k: f"{v:.1e}" for k, v in {**errs, **gerrs}.items()})
    assert max(errs.values()) <= 1e-6, errs
    assert max(gerrs.values()) <= 1e-5, gerrs
    # float64 operands run the same graph in float64 (1 - exp(-s) alone costs fp32 an eps / s relative error, s ~ 1e-3 here: no tight bar)
    s64 = R.coarse_stage(st["sig_c"].double(), st["rgb_c"].double(), st["t_c"], st["near"], st["far"], o["delta0"], Nf, st["k"])
    assert all(v.dtype == torch.float64 for v in s64.values()) and R.l2_rel(s["w"], s64["w"]) < 1e-4


def test_merged_reference_is_the_oracles_graph(oracle, stages):
    st, Nc, Nf = stages, stages["Nc"], stages["Nf"]
    B, N = st["t_c"].shape[0], Nc + Nf
    gen = torch.Generator().manual_seed(4)
    dC_f = torch.randn(B, 3, generator=gen)
    g_m = torch.randn(B, 4, generator=gen)
    leaves = {k: st[k].clone().requires_grad_(True) for k in ("sig_c", "sig_f", "rgb_c", "rgb_f", "t_f")}
    bundle = torch.cat((torch.cat((st["t_c"], leaves["t_f"]), 1).unsqueeze(2), torch.cat((leaves["rgb_c"], leaves["rgb_f"]), 1),
                        torch.cat((leaves["sig_c"], leaves["sig_f"]), 1).unsqueeze(2)), dim=2)
    sb = torch.gather(bundle, 1, st["perm"])  # (the oracle's own sort order, replayed so that ties cannot differ)
    delta = torch.cat((sb[:, 1:, 0] - sb[:, :-1, 0], torch.full((B, 1), R.LAST)), dim=1)
    w = oracle.weights_from_sigma(delta, sb[:, :, 4])
    C_f = oracle.composite(w, sb[:, :, 1:4])
    D_f, A_f = (w * sb[:, :, 0]).sum(1), w.sum(1)
    ((C_f * dC_f).sum() + (D_f * g_m[:, 2]).sum() + (A_f * g_m[:, 3]).sum()).backward()
    assert torch.equal(sb.detach(), torch.cat((st["t_s"].unsqueeze(2), st["rgb_s"], st["sig_s"].unsqueeze(2)), 2))
    with torch.no_grad():
        m = R.merged_composite(st["t_s"], st["rgb_s"], st["sig_s"])
    errs = {n: R.l2_rel(m[n], ref.detach()) for n, ref in (("w", w), ("C_f", C_f), ("D_f", D_f), ("A_f", A_f))}
    got = R.merged_grads(sb.detach(), st["perm"].permute(0, 2, 1), Nc, dC_f, torch.float32, g_m)
    gerrs = {n: R.l2_rel(a, leaves[n].grad) for n, a in zip(("sig_c", "sig_f", "rgb_c", "rgb_f", "t_f"), got)}
    print({k: f"{v:.1e}" for k, v in {**errs, **gerrs}.items()})
    assert max(errs.values()) <= 1e-6, errs
    assert max(gerrs.values()) <= 1e-5, gerrs


def test_decision_replica_takes_the_oracles_bins(stages):
    st = stages
    d = R.decision_replica(st["w_c"], st["Nf"])
    assert torch.equal(d["cdf"], st["cdf"]) and torch.equal(d["u"], st["u"])
    assert torch.equal(d["k"], st["k"]) and torch.equal(d["bad"], st["bad"])
    assert float(d["ambiguous"].float().mean()) <= R.AMBIGUOUS_MAX


def _replica_of_case(oracle, Nc, Nf):
    o = R.operands(Nc, Nf)
    w32 = oracle.weights_from_sigma(((o["far"] - o["near"]) / Nc)[:, None].expand(-1, Nc), o["sig_c"])
    return o, R.decision_replica(w32, Nf)


@pytest.mark.parametrize("Nc,Nf", list(R.CASES))
def test_operands_are_what_the_gpu_tests_assume(oracle, Nc, Nf):
    o, d = _replica_of_case(oracle, Nc, Nf)
    n = int(d["ambiguous"].sum())
    print(f"({Nc}, {Nf}): {n} of {d['ambiguous'].numel()} fine samples ambiguous")
    assert n <= R.AMBIGUOUS_MAX * d["ambiguous"].numel()
    if (Nc, Nf) == (5, 3):
        assert bool(d["bad"].any())  # Nc > Nf: a bin index above Nf - 1, the condition of quirk Q7
    assert o["sig_c"].dtype == torch.float32 and o["t_c"].shape == (R.B_RAYS, Nc)
    zeros = float((o["sig_c"] == 0).float().mean())
    assert Nc < 31 or 0.35 < zeros < 0.65  # about half exact zeros
    tau = (o["sig_c"] * ((o["far"] - o["near"]) / Nc)[:, None]).sum(1)
    if Nc >= 31:
        for b in range(R.B_RAYS):
            assert math.isclose(float(tau[b]), R.DEPTHS[b], rel_tol=1e-3)
        with torch.no_grad():
            s = R.coarse_stage(o["sig_c"].double(), o["rgb_c"].double(), o["t_c"], o["near"], o["far"], o["delta0"], Nf, d["k"])
        T = torch.exp(-torch.cumsum(o["sig_c"] * ((o["far"] - o["near"]) / Nc)[:, None], 1))
        assert float(T[4:, -1].max()) < 1e-20 and float(s["A_c"][:2].max()) < 0.11  # opaque rays underflow fp32's weights, thin ones stay thin


def test_stable_order():
    gen = torch.Generator().manual_seed(0)
    x = torch.round(torch.randn(4, 97, generator=gen) * 2)
    x[:, ::7] = float("nan")
    x[:, 3::11] = -torch.tensor(float("nan"))
    x[:, 5::9] = -0.0
    x[:, 6::13] = 0.0
    got = R.stable_order(x)
    for r in range(x.shape[0]):
        key = lambda i: (1, 0.0) if math.isnan(float(x[r, i])) else (0, float(x[r, i]) + 0.0)
        assert got[r].tolist() == sorted(range(x.shape[1]), key=key)  # (Python's sort is stable; -0.0 == 0.0)


def test_stage_entry_points_are_declared_and_bound(pkg):
    with open(os.path.join(ROOT, "include", "nerf_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+NERF_HIP_ABI_VERSION\s+7\b", hdr) and pkg._abi.NERF_HIP_ABI_VERSION == 7
    section = hdr[hdr.index("Stage entry points"):]
    for name in NEW_EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", section), name
        assert name in pkg._abi.EXPORTS, name
        assert name in hdr[:hdr.index("enum {")], name  # listed in the version comment's "later additions under 7"
    for fn in ("coarse_composite_maps", "coarse_composite_backward_add", "merge_composite_train", "merge_composite_backward"):
        assert callable(getattr(pkg.ops, fn))
