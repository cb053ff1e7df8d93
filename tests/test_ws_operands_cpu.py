"""CPU checks of tests/ws_operands.py, the operand reader and float64 reference the weight-gradient tests rest on: the vectorised
fragment decoder against the layout's element-by-element definition, the reference's 24 formulas (fold included) against autograd
through the layers they differentiate, and the schedule restatement of tests/test_gpu_weight_gradients.py at the sizes DESIGN.md names."""
import os

import torch

import ws_operands as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ks_tables_match_the_header():
    txt = open(os.path.join(ROOT, "nerf-tiny_amd", "csrc", "bf16_common.h")).read()
    assert "constexpr int BS_GP = 0, BS_H0 = 1, BS_C = 9, BS_GD = 10, NBS = 11;" in txt
    assert "t == BS_GP ? 4 : t < BS_C ? 16 : t == BS_C ? 8 : 2" in txt
    assert "constexpr int BG_L0 = 0, BG_D = 8, BG_Z = 9, NBG = 10;" in txt
    assert "t < BG_D ? 16 : t == BG_D ? 8 : 2" in txt
    assert W.BS_KS == [4 if t == W.BS_GP else 16 if t < W.BS_C else 8 if t == W.BS_C else 2 for t in range(11)]
    assert W.BG_KS == [16 if t < W.BG_D else 8 if t == W.BG_D else 2 for t in range(10)]


def test_decode_matches_the_layout_definition():
    wb_tot = 3
    gen = torch.Generator().manual_seed(0)
    buf = torch.randint(0, 256, (wb_tot * sum(W.BS_KS) * W.FRAG_BYTES,), dtype=torch.uint8, generator=gen)
    for t in (W.BS_GP, W.BS_H0 + 2, W.BS_C, W.BS_GD):
        ks_t = W.BS_KS[t]
        start = wb_tot * W.FRAG_BYTES * sum(W.BS_KS[:t])
        raw = buf[start:start + wb_tot * ks_t * W.FRAG_BYTES].view(torch.bfloat16)
        want = torch.empty(wb_tot * 32, ks_t * 16, dtype=torch.bfloat16)
        for wb in range(wb_tot):
            for ks in range(ks_t):
                for h in range(2):
                    for j in range(32):
                        for s in range(8):
                            want[wb * 32 + j, 16 * ks + 4 * h + (s & 3) + 8 * (s >> 2)] = raw[((wb * ks_t + ks) * 64 + h * 32 + j) * 8 + s]
        got = W.decode(buf, wb_tot, W.BS_KS, t)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), t


def _random_ops(n, gen):
    shapes = {"gp": 60, "c": 128, "gd": 24, "gdir": 128, "dz": 3, "dspre": 1}
    shapes.update({f"h{l}": 256 for l in range(8)})
    shapes.update({f"g{l}": 256 for l in range(8)})
    return {k: (torch.randn(n, f, generator=gen, dtype=torch.float64),) for k, f in shapes.items()}


def test_reference_is_the_gradient_of_the_layers():
    """sum over layers of <X W^T + b, G> differentiated by autograd gives exactly the 24 tensors dw_reference forms, the fold of
    point_info into dir_info included (feat = h7 W_pi^T + b_pi, dir_info's input = [gamma_d | feat])."""
    gen = torch.Generator().manual_seed(1)
    ops = _random_ops(40, gen)
    shapes = [(256, 60), (256,)] + [(256, 256), (256,)] * 3 + [(256, 316), (256,)] + [(256, 256), (256,)] * 3 + \
             [(1, 256), (1,), (256, 256), (256,), (128, 280), (128,), (3, 128), (3,)]
    w = [torch.randn(*s, generator=gen, dtype=torch.float64, requires_grad=True) for s in shapes]
    o = {k: v[0] for k, v in ops.items()}
    lin = lambda x, i: x @ w[i].T + w[i + 1]
    loss = 0
    for l in range(8):
        x = o["gp"] if l == 0 else torch.cat((o["h3"], o["gp"]), 1) if l == 4 else o[f"h{l - 1}"]
        loss = loss + (lin(x, 2 * l) * o[f"g{l}"]).sum()
    loss = loss + (lin(o["h7"], W.W_SIGMA) * o["dspre"]).sum()
    feat = lin(o["h7"], W.W_PI)
    loss = loss + (lin(torch.cat((o["gd"], feat), 1), W.W_DIR) * o["gdir"]).sum()
    loss = loss + (lin(o["c"], W.W_COLOR) * o["dz"]).sum()
    loss.backward()
    ref = W.dw_reference(ops, [p.detach() for p in w])
    for i, (p, (r, mag)) in enumerate(zip(w, ref)):
        assert r.shape == p.shape and mag.shape == p.shape, i
        assert float((r - p.grad).norm() / p.grad.norm()) < 1e-12, i
        assert bool((mag >= r.abs() * (1 - 1e-12)).all()), i


def test_split_reference_is_the_three_kernel_products():
    """hi.hi + hi.mid + mid.hi for the products, hi + mid for the column sums; a zero mid part gives the one-part reference."""
    gen = torch.Generator().manual_seed(2)
    hi, mid = _random_ops(16, gen), _random_ops(16, gen)
    w = [torch.randn(s, generator=gen, dtype=torch.float64) for s in [(128, 280), (256, 256), (256,)]]
    weights = [None] * 18 + [w[1], w[2], w[0]] + [None] * 3
    two = W.dw_reference({k: hi[k] + mid[k] for k in hi}, weights)
    one = W.dw_reference(hi, weights)
    zero = W.dw_reference({k: hi[k] + (torch.zeros_like(hi[k][0]),) for k in hi}, weights)
    for (a, _), (b, _) in zip(one, zero):
        assert torch.allclose(a, b, rtol=1e-13, atol=0)
    g, x, gm, xm = hi["g2"][0], hi["h1"][0], mid["g2"][0], mid["h1"][0]
    assert torch.allclose(two[4][0], g.T @ x + g.T @ xm + gm.T @ x, rtol=1e-12)
    assert torch.allclose(two[5][0], (g + gm).sum(0), rtol=1e-12)


def test_schedule_restatement_at_the_documented_sizes():
    import test_gpu_weight_gradients as T

    # DESIGN.md / the issue table: ray duty on at 1024 and 4096 rays, off at 400, 512, 853 (64 + 128)
    assert [T.dw_ray_duty_ok(B, 64, 128) for B in (1024, 4096, 400, 512, 853)] == [True, True, False, False, False]
    # the multi launch up to 5120 wave blocks: 852 rays below, 853 above
    assert W.wave_blocks(852, 64) + W.wave_blocks(852, 128) == 5112 and W.wave_blocks(853, 64) + W.wave_blocks(853, 128) == 5128
    assert [T.expected_path("bf16_mlp", 852, 64, 128, e) for e in (False, True)] == ["a", "b"]
    assert [T.expected_path("split_train", 853, 64, 128, e) for e in (False, True)] == ["c", "d"]
