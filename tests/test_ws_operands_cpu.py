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


# ---- the forward and the dX chain (tests/test_gpu_layers.py) ---------------------------------------------------------------------
def test_fp32_mask_decoder_inverts_the_image():
    gen = torch.Generator().manual_seed(3)
    tiles = 3
    hidden = [torch.randn(tiles * 64 - 5, 256, generator=gen, dtype=torch.float64) for _ in range(8)]
    got = W.decode_relu_masks(W.relu_mask_image(hidden, tiles))
    for l in range(8):
        assert torch.equal(got[l, :tiles * 64 - 5], hidden[l] > 0), l
        assert not bool(got[l, tiles * 64 - 5:].any())
    # and the other way round: any bit pattern survives decode -> image
    img = torch.randint(-32768, 32768, (8, tiles, 4, 256), generator=gen, dtype=torch.int32).to(torch.int16)
    assert torch.equal(W.relu_mask_image([m.double() for m in W.decode_relu_masks(img)], tiles), img)


def test_bmask_decoder_matches_the_layout_definition():
    wb_tot = 2
    gen = torch.Generator().manual_seed(4)
    words = torch.randint(-32768, 32768, (W.BM_LAYERS * wb_tot * 64 * 8,), generator=gen, dtype=torch.int32).to(torch.int16)
    got = W.decode_bmask(words, wb_tot)
    u = words.to(torch.int32) & 0xffff
    want = torch.zeros(W.BM_LAYERS, wb_tot * 32, 256, dtype=torch.bool)
    for l in range(W.BM_LAYERS):
        for wb in range(wb_tot):
            for lane in range(64):
                j, h = lane & 31, lane >> 5
                for f in range(8):
                    word = int(u[((l * wb_tot + wb) * 64 + lane) * 8 + f])
                    for r in range(16):
                        want[l, wb * 32 + j, 32 * f + 8 * (r >> 2) + 4 * h + (r & 3)] = bool((word >> (15 - r)) & 1)
    assert torch.equal(got, want)


def _params(gen):
    import nerf_oracle

    w = nerf_oracle.make_weights(6, sharp=True)
    return {k: v.double() for k, v in w.items()}, [v.double() for v in w.values()]


def test_layer_reference_reproduces_the_oracle_mlp_in_float64():
    """From the oracle's own hidden layers as the saved inputs, every layer of layer_reference (the fold in float64 included) is the
    oracle's float64 forward; the magnitudes bound the values."""
    import nerf_oracle

    gen = torch.Generator().manual_seed(5)
    p, weights = _params(gen)
    n = 50
    gp, gd = torch.randn(n, 60, generator=gen, dtype=torch.float64), torch.randn(n, 24, generator=gen, dtype=torch.float64)
    rgb, sigma, hidden, feat, c = nerf_oracle.mlp(p, gp, gd, return_hidden=True)
    ops = {"gp": (gp,), "gd": (gd,), "c": (c,)}
    ops.update({f"h{l}": (h,) for l, h in enumerate(hidden)})
    Wd = p["network.dir_info.0.weight"]
    ops["start"] = (p["network.dir_info.0.bias"] + gd @ Wd[:, :24].T + Wd[:, 24:] @ p["network.point_info.bias"],)
    ref = W.layer_reference(ops, weights, "fp32")
    want = {f"h{l}": h for l, h in enumerate(hidden)}
    want.update({"sigma": sigma, "c": c, "rgb": rgb})
    for k, v in want.items():
        got, mag, _ = ref[k]
        assert float((got - v).abs().max() / v.abs().max()) < 1e-12, k
        assert bool((mag * (1 + 1e-12) >= (ref[k][2].abs() if k != "rgb" else 0)).all()), k
    # bf16 / split modes with the workspace's fold and bias: the same graph with the device's W_fold (here the exact one)
    Wfold = Wd[:, 24:] @ p["network.point_info.weight"]
    ops.update({"fold": (Wfold,), "b_fold": (Wd[:, 24:] @ p["network.point_info.bias"],)})
    for mode in ("bf16", "split"):
        r = W.layer_reference({k: v if k in W.NOT_ROWS or mode == "bf16" else v + (torch.zeros_like(v[0]),) for k, v in ops.items()},
                              [W.rne_bf16(x) if mode == "bf16" else x for x in weights], mode)
        assert r["c"][0].shape == c.shape and r["rgb"][0].shape == rgb.shape


def test_chain_reference_is_autograd_through_the_same_graph():
    """Each layer of chain_reference against autograd of <layer(x), g_next> with respect to the layer's input, masked."""
    gen = torch.Generator().manual_seed(6)
    p, weights = _params(gen)
    n = 40
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    ops = {"dz": (r(n, 3),), "dspre": (r(n, 1),), "gdir": (r(n, 128),)}
    ops.update({f"g{l}": (r(n, 256),) for l in range(8)})
    ops.update({f"m{l}": (r(n, 256) > 0,) for l in range(8)})
    ops["mc"] = (r(n, 128) > 0,)
    ref = W.chain_reference(ops, weights, "fp32")
    Wd, Wpi = p["network.dir_info.0.weight"], p["network.point_info.weight"]

    def grad(f, x, g):
        x = x.clone().requires_grad_(True)
        (f(x) * g).sum().backward()
        return x.grad

    o = {k: v[0] for k, v in ops.items()}
    want = {"gdir": grad(lambda c: c @ p["network.color_layer.0.weight"].T, torch.zeros(n, 128, dtype=torch.float64), o["dz"]) * o["mc"]}
    h7 = torch.zeros(n, 256, dtype=torch.float64)
    want["g7"] = (grad(lambda h: (h @ Wpi.T) @ Wd[:, 24:].T, h7, o["gdir"]) +
                  grad(lambda h: h @ p["network.sigma_layer.0.weight"].T, h7, o["dspre"])) * o["m7"]
    for l in range(6, -1, -1):
        Wn = p[f"network.point_layer.{l + 1}.0.weight"]
        want[f"g{l}"] = grad(lambda h: h @ Wn[:, :256].T, h7, o[f"g{l + 1}"]) * o[f"m{l}"]
    for k, v in want.items():
        got, mag = ref[k]
        assert float((got - v).abs().max() / v.abs().max()) < 1e-12, k
        assert bool((mag * (1 + 1e-12) >= got.abs()).all()), k


def test_rne_helper_agrees_with_torch_on_fp32_inputs():
    """Every fp32 bit pattern of a few exponent ranges (and exact ties) rounds as torch's fp32 -> bf16 conversion does."""
    for e in (0x3f, 0x40, 0x01, 0x00, 0x7e, 0xc2):
        bits = (torch.arange(1 << 23, dtype=torch.int64) | (e << 23)).to(torch.int32)
        x = bits.view(torch.float32)
        want = x.to(torch.bfloat16).to(torch.float64)
        assert torch.equal(W.rne_bf16(x.double()), want), hex(e)
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -126 * (1 + 2.0 ** -8)], dtype=torch.float64)
    assert W.rne_bf16(ties).tolist() == [1.0, 1 + 2 * 2.0 ** -7, -1.0, 2.0 ** -126]
    assert torch.equal(W.rne_bf16(ties), ties.float().to(torch.bfloat16).double())


def test_bf16_interval_accepts_an_accumulation_within_E_and_rejects_truncation():
    import test_gpu_layers as T

    gen = torch.Generator().manual_seed(7)
    ref = torch.randn(200000, generator=gen, dtype=torch.float64)
    mag = ref.abs() * 4 + 1
    for relu in (False, True):
        f = (lambda x: x.clamp_min(0)) if relu else (lambda x: x)
        for s in (-1, 1, 0):
            acc = ref + s * T.E_BF16 * mag  # an accumulation E mag off (or exact)
            dev = W.rne_bf16(f(acc)).to(torch.bfloat16)
            assert bool(T.bf16_interval_ok(dev, ref, mag, relu).all())
            assert float(T.ratio("bf16", (dev,), ref, mag, relu).max()) <= 1.0 + 1e-9
        bad = W.trunc_bf16(f(ref)).to(torch.bfloat16)
        assert not bool(T.bf16_interval_ok(bad, ref, mag, relu).all())
        assert float(T.ratio("bf16", (W.rne_bf16(f(ref)).to(torch.bfloat16),), ref, mag, relu, rnd="trunc").max()) > T.TEETH
