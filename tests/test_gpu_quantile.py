"""GPU: the per-ray quantile depths (rule QD of include/nerf_hip.h) -- the quantile forms of k_coarse_x / k_merge_x through their stage entries and
through nerf_hip_forward_quantiles, NeRFModel.render(maps=True, quantiles=) and fuse_depth(depth_stat=, max_spread=).

  * every output a quantile call shares with the maps call has that call's bits;
  * the quantile depths are BIT-IDENTICAL to the numpy restatement (tests/quantile_reference.py) evaluated on the call's own fp32 weights
    and depths -- the rule fixes the order of the fp64 prefix sums, so no tolerance enters;
  * hand-made rays (two layers, nothing hit, a hit in element 0 of the second 64-chunk, all weight in the last sample) land where the
    rule says;
  * a constant field against the fp64 definition over the call's own depths, to 1e-3 of the coarse sample spacing (derived in the test);
  * every refusal is NERF_HIP_ERR_ARG and leaves the outputs' sentinels in place;
  * the Python layers keep render's batch semantics and fuse what the test builds by hand.
"""
import ctypes

import numpy as np
import pytest
import torch

import quantile_reference as QR
import ray_stage_reference as R
import tsdf_reference as TR
from conftest import load_golden
from nerf_oracle import coarse_depths

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = -7.0
QSETS = {1: (0.5,), 3: (0.25, 0.5, 0.75), 4: (0.1, 0.25, 0.5, 0.9)}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _restated(w, t, q):
    """the restatement on device tensors w, t [B, N] -> a CPU fp32 tensor [B, nq]"""
    return torch.from_numpy(QR.quantile_depths(w.cpu().numpy(), t.cpu().numpy(), q))


# ---------------------------------------------------------------------------------------------------------------
# coarse stage
# ---------------------------------------------------------------------------------------------------------------
B_COARSE, NF_COARSE = 7, 8  # 7 rays: the second workgroup of four waves has one wave behind the batch


def _coarse_operands(Nc, dev):
    if Nc == 1:  # (the maps entry's minimum is Nc = 2: a one-sample ray has no spacing; delta0 is given)
        gen = torch.Generator().manual_seed(1)
        near = 2.0 + torch.rand(B_COARSE, generator=gen)
        o = dict(near=near, far=near + 3.0, t_c=near[:, None].clone(), delta0=0.1, sig_c=torch.rand(B_COARSE, 1, generator=gen) * 0.5,
                 rgb_c=torch.rand(B_COARSE, 1, 3, generator=gen))
        o["sig_c"][2] = 0.0
    else:
        o = R.operands(Nc, NF_COARSE, seed=Nc, B=B_COARSE)
    return o, {k: v.to(dev).contiguous() for k, v in o.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("nq", [1, 3, 4])
@pytest.mark.parametrize("Nc", [1, 2, 63, 64, 65, 130, 200])
def test_coarse_stage(pkg, dev, Nc, nq):
    q = QSETS[nq]
    o, d = _coarse_operands(Nc, dev)
    args = (d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], NF_COARSE)
    w, C, t_f, st, M, Q = pkg.ops.coarse_composite_quantiles(*args, q, sentinel=SENTINEL)
    assert Q.shape == (B_COARSE, 2, nq)
    if Nc >= 2:  # every shared output: the maps call's bits
        w0, C0, t0, st0, M0 = pkg.ops.coarse_composite_maps(*args)
        assert _same(w, w0) and _same(C, C0) and _same(t_f, t0) and st == st0
        assert _same(M[:, :2], M0[:, :2]) and bool(torch.isnan(M[:, 2:]).all())
    else:  # one sample: every sum has one term, so the outputs are exact functions of the one weight
        assert bool(torch.isfinite(w).all()) and bool((w[:, 0] > 0).sum() == B_COARSE - 1) and float(w[2, 0]) == 0.0
        assert _same(C, w * d["rgb_c"][:, 0]) and _same(M[:, 0], w[:, 0] * d["t_c"][:, 0]) and _same(M[:, 1], w[:, 0])
    want = _restated(w, d["t_c"], q)
    assert _same(Q[:, 0].cpu(), want), (Q[:, 0].cpu(), want)
    assert bool((Q[:, 1] == SENTINEL).all())  # the fine row is not this kernel's
    t_lo, t_hi = d["t_c"][:, :1], d["t_c"][:, -1:]
    assert bool((Q[:, 0] >= t_lo).all()) and bool((Q[:, 0] <= t_hi).all()) and bool((Q[:, 0, 1:] >= Q[:, 0, :-1]).all())
    # the rays behind the batch store nothing: a 5-ray call into 7-ray buffers (three waves of the second workgroup idle)
    w5, C5, t5, _, M5, Q5 = pkg.ops.coarse_composite_quantiles(*args, q, sentinel=SENTINEL, rays=5)
    assert _same(Q5[:5], Q[:5]) and bool((Q5[5:] == SENTINEL).all()) and _same(w5[:5], w[:5]) and bool(torch.isnan(M5[5:]).all())


# ---------------------------------------------------------------------------------------------------------------
# merge stage
# ---------------------------------------------------------------------------------------------------------------
MERGE_SIZES = [(64, 128), (16, 32), (24, 40), (65, 63), (1, 1), (300, 340)]  # registers; LDS P = 64; a padded P; ties, LDS P = 128; P = 2; P = 1024
B_MERGE = 5


def _merge_operands(Nc, Nf, dev):
    if (Nc, Nf) == (65, 63):
        o = R.tie_operands(B=B_MERGE)
    else:
        gen = torch.Generator().manual_seed(100 * Nc + Nf)
        near = 2.0 + torch.rand(B_MERGE, generator=gen)
        far = near + 3.0 + 2.0 * torch.rand(B_MERGE, generator=gen)
        u = torch.linspace(0, 1, Nc)[None] if Nc > 1 else torch.zeros(1, 1)
        t_c = near[:, None] + (far - near)[:, None] * u
        t_f = near[:, None] + (far - near)[:, None] * torch.rand(B_MERGE, Nf, generator=gen)
        depth = torch.tensor([R.DEPTHS[b % len(R.DEPTHS)] for b in range(B_MERGE)])
        scale = depth / (far - near) * 2.0  # relu(randn) averages 0.4: total optical depths about DEPTHS
        o = dict(t_c=t_c, t_f=t_f, sig_c=torch.relu(torch.randn(B_MERGE, Nc, generator=gen)) * scale[:, None],
                 sig_f=torch.relu(torch.randn(B_MERGE, Nf, generator=gen)) * scale[:, None],
                 rgb_c=torch.sigmoid(torch.randn(B_MERGE, Nc, 3, generator=gen)), rgb_f=torch.sigmoid(torch.randn(B_MERGE, Nf, 3, generator=gen)))
    return {k: v.to(dev).contiguous() for k, v in o.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("joint,perm", [(0, True), (0, False), (1, True)])
@pytest.mark.parametrize("Nc,Nf", MERGE_SIZES)
def test_merge_stage(pkg, dev, Nc, Nf, joint, perm):
    d = _merge_operands(Nc, Nf, dev)
    args = (d["t_c"], d["t_f"], d["sig_c"], d["sig_f"], d["rgb_c"], d["rgb_f"])
    b0, w0, C0, p0, M0 = pkg.ops.merge_composite_train(*args, last=R.LAST, joint=bool(joint), maps=True)
    for nq in (1, 3, 4):
        q = QSETS[nq]
        b, w, C, p, M, Q = pkg.ops.merge_composite_quantiles(*args, q, last=R.LAST, joint=bool(joint), perm=perm, sentinel=SENTINEL)
        assert _same(b, b0) and _same(w, w0) and _same(C, C0) and _same(M[:, 2:], M0[:, 2:]) and bool(torch.isnan(M[:, :2]).all())
        assert (p is None) if not perm else torch.equal(p, p0)
        want = _restated(w, b[:, :, 0], q)
        assert _same(Q[:, 1].cpu(), want), (Q[:, 1].cpu(), want)
        assert bool((Q[:, 0] == SENTINEL).all())  # the coarse row is not this kernel's
        assert bool((Q[:, 1] >= b[:, :1, 0]).all()) and bool((Q[:, 1] <= b[:, -1:, 0]).all()) and bool((Q[:, 1, 1:] >= Q[:, 1, :-1]).all())


# ---------------------------------------------------------------------------------------------------------------
# hand-made rays through both stages
# ---------------------------------------------------------------------------------------------------------------
IA, IB = 20, 100  # the two layers' samples (of 130: one in the first 64-chunk, one in the second)


def _hand_s(N):
    """[5, N] optical depths s = sigma * delta: two layers (front share 0.3, 0.7), nothing, a hit in sample 64 alone, the last sample alone"""
    s = np.zeros((5, N))
    for r, a in ((0, 0.3), (1, 0.7)):
        s[r, IA], s[r, IB] = QR.two_layer_s(a)
    s[3, 64] = 5.0
    s[4, N - 1] = 1.0
    return s


def _check_hand(Q, t, mean, q):
    """Q [5, 3] at q = (0.25, 0.5, 0.75), t [5, N] the samples in the composite's order (CPU tensors), mean [5] = D / A"""
    N = t.shape[1]
    step = lambda r, i: float(t[r, i + 1] - t[r, i])
    assert abs(float(Q[0, 1] - t[0, IB])) <= step(0, IB) and abs(float(Q[1, 1] - t[1, IA])) <= step(1, IA)  # the median stays on a layer
    for r in (0, 1):  # ... and the mean lies strictly between them, several samples from either
        assert float(t[r, IA + 4]) < float(mean[r]) < float(t[r, IB - 4])
    assert bool((Q[2] == t[2, N - 1]).all())  # nothing hit: the last sample (A = 0 says so)
    want = [F32(np.float64(t[3, 64]) + np.float64(F32(x)) * (np.float64(t[3, 65]) - np.float64(t[3, 64]))) for x in q]
    assert Q[3].numpy().tobytes() == np.array(want, F32).tobytes()  # E = the carry = 0 and theta / w_64 = q exactly
    assert bool((Q[4] == t[4, N - 1]).all())  # all weight in the last sample: never extrapolated


def test_hand_made_rays_coarse(pkg, dev):
    Nc, q = 130, QSETS[3]
    near = torch.tensor([2.0, 2.5, 2.0, 3.0, 2.25])
    far = near + torch.tensor([4.0, 3.0, 5.0, 4.0, 3.5])
    t_c = coarse_depths(near, far, Nc)
    delta_c = ((far - near) / Nc).double()[:, None]
    sig = (torch.from_numpy(_hand_s(Nc)) / delta_c).float()
    rgb = torch.full((5, Nc, 3), 0.5)
    w, C, t_f, st, M, Q = pkg.ops.coarse_composite_quantiles(t_c.to(dev), sig.to(dev), rgb.to(dev), near, far, float(t_c[0, 1] - t_c[0, 0]), 8, q)
    assert _same(Q[:, 0].cpu(), _restated(w, t_c, q))
    M = M.cpu()
    assert float(M[2, 1]) == 0.0 and bool((M[(0, 1, 3, 4), 1] > 0).all())
    share = (w[:2, IA] / w[:2].sum(1)).cpu()
    assert abs(float(share[0]) - 0.3) < 1e-4 and abs(float(share[1]) - 0.7) < 1e-4
    _check_hand(Q[:, 0].cpu(), t_c, M[:, 0] / M[:, 1], q)


def test_hand_made_rays_merged(pkg, dev):
    """the same five rays through the joint sort (the samples keep their sigma): 64 coarse + 66 fine samples dealt out of 130 sorted depths"""
    Nc, Nf, q = 64, 66, QSETS[3]
    N = Nc + Nf
    gen = torch.Generator().manual_seed(5)
    t = torch.sort(2.0 + 4.0 * torch.rand(5, N, generator=gen), dim=1).values
    delta = torch.cat((t[:, 1:] - t[:, :-1], torch.full((5, 1), R.LAST)), 1).double()
    sig = (torch.from_numpy(_hand_s(N)) / delta).float()
    deal = torch.randperm(N, generator=gen)
    ic, jf = deal[:Nc], deal[Nc:]
    rgb = torch.full((5, N, 3), 0.5)
    dd = lambda x: x.contiguous().to(dev)
    b, w, C, p, M, Q = pkg.ops.merge_composite_quantiles(dd(t[:, ic]), dd(t[:, jf]), dd(sig[:, ic]), dd(sig[:, jf]), dd(rgb[:, ic]), dd(rgb[:, jf]), q,
                                                         last=R.LAST, joint=True)
    assert torch.equal(b[:, :, 0].cpu(), t) and torch.equal(b[:, :, 4].cpu(), sig)
    assert _same(Q[:, 1].cpu(), _restated(w, b[:, :, 0], q))
    M = M.cpu()
    assert float(M[2, 3]) == 0.0 and bool((M[(0, 1, 3, 4), 3] > 0).all())
    share = (w[:2, IA] / w[:2].sum(1)).cpu()
    assert abs(float(share[0]) - 0.3) < 1e-4 and abs(float(share[1]) - 0.7) < 1e-4
    _check_hand(Q[:, 1].cpu(), t, M[:, 2] / M[:, 3], q)


# ---------------------------------------------------------------------------------------------------------------
# the whole call
# ---------------------------------------------------------------------------------------------------------------
MODES = {  # name -> (flags, rays): tests/test_gpu_maps.py's
    "fp32": (0, 256),
    "tile": (1 << 1, 256),
    "split": (1 << 4, 256),
    "bf16_pair": (1 << 2, 256),
    "bf16_large": (1 << 2, 1024),
    "corrected": (1 << 5, 256),
}
SAMPLES = [(64, 128), (16, 32)]


def _call(pkg, P, row, col, pb, K, Nc, Nf, flags, q=None, nq=None, null=(), sentinel=float("nan")):
    """One direct nerf_hip_forward_maps (q None) / nerf_hip_forward_quantiles call on a fresh workspace -> (rc, C_c, C_f, maps, Q, status, ws).
    nq: the count handed over (default len(q)); null: names of arguments handed over as NULL ("q", "qdepth", "maps")."""
    _abi = pkg._abi
    dev = P[0].device
    B = row.shape[0]
    n = _abi.ws_bytes(B, Nc, Nf, flags & ~_abi.SAVE_FOR_BACKWARD)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    Cc, Cf, M = (torch.full((B, k), sentinel, device=dev) for k in (3, 3, 4))
    K9 = _abi.f32_array(K.reshape(-1).tolist())
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, None, B, Nc, Nf, pkg.nerf.LAST_DELTA, Cc.data_ptr(), Cf.data_ptr(),
            None if "maps" in null else M.data_ptr(), ws.data_ptr(), n, flags, stream)
    Q = None
    if q is None:
        rc = _abi.lib().nerf_hip_forward_maps(*args)
    else:
        Q = torch.full((B, 2, max(len(q), 1)), sentinel, device=dev)
        rc = _abi.lib().nerf_hip_forward_quantiles(*args, None if "q" in null else _abi.f32_array(q), len(q) if nq is None else nq,
                                                   None if "qdepth" in null else Q.data_ptr())
    st = ctypes.c_uint32(0)
    if rc == 0:
        _abi.check(_abi.lib().nerf_hip_read_status(ws.data_ptr(), n, ctypes.byref(st), stream))
    return rc, Cc, Cf, M, Q, int(st.value), ws


def _weights_dev(oracle, seed, sharp, dev):
    p = oracle.make_weights(seed, sharp)
    return p, [v.to(dev).contiguous() for v in p.values()]


def _inputs(oracle, B, dev, seed=3):
    row, col, pb, K, _ = oracle.fern_inputs(B, seed=seed)  # per-image near / far
    return row.to(dev).contiguous(), col.to(dev).contiguous(), pb.float().to(dev).contiguous(), K


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_quantiles_against_forward_maps(oracle, pkg, dev, mode, Nc, Nf):
    flags, B = MODES[mode]
    q = QSETS[4]
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K = _inputs(oracle, B, dev)
    rc0, c0, f0, M0, _, s0, _ = _call(pkg, P, row, col, pb, K, Nc, Nf, flags)
    rc1, c1, f1, M1, Q, s1, ws = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, q=q)
    torch.cuda.synchronize()
    assert rc0 == 0 and rc1 == 0
    assert _same(c0, c1) and _same(f0, f1) and _same(M0, M1) and s0 == s1
    assert bool(torch.isfinite(Q).all())
    view = lambda name, n: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, (B, n))
    t_c, t_f, w_c = view("t_c", Nc), view("t_f", Nf), view("w_c", Nc)
    near, far = pb[:, 15:16], pb[:, 16:17]
    Qc, Qf = Q[:, 0], Q[:, 1]
    assert bool((Qc >= near).all()) and bool((Qc <= far).all()) and bool((Qc[:, 1:] >= Qc[:, :-1]).all())
    t_all = torch.cat((t_c, t_f), 1)
    assert bool((Qf >= t_all.min(1, keepdim=True).values).all()) and bool((Qf <= t_all.max(1, keepdim=True).values).all())
    assert bool((Qf[:, 1:] >= Qf[:, :-1]).all())
    assert _same(Qc.cpu(), _restated(w_c, t_c, q))  # the coarse row: the rule on the call's own workspace weights


def _weights_fp64(delta, sigma):
    s = delta * sigma
    return torch.exp(-torch.cumsum(s, 1)) * (1.0 - torch.exp(-s))


def _definition_fp64(w, t, q):
    """rule QD over fp64 weights and depths [B, N] (sequential sums), q fp32 -> [B, nq] fp64"""
    w, t = w.numpy(), t.numpy()
    out = np.empty((w.shape[0], len(q)))
    for b in range(w.shape[0]):
        Wi = np.cumsum(w[b])
        for j, x in enumerate(q):
            theta = float(F32(x)) * Wi[-1]
            k = int(np.nonzero(Wi >= theta)[0][0])
            f = min(max((theta - (Wi[k - 1] if k else 0.0)) / w[b, k], 0.0), 1.0)
            out[b, j] = t[b, k] + f * ((t[b, k + 1] if k + 1 < w.shape[1] else t[b, k]) - t[b, k])
    return out


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("mode", ["fp32", "split", "bf16_large", "corrected"])
def test_constant_field_against_the_fp64_definition(oracle, pkg, dev, mode, Nc, Nf):
    """Every weight zero and the sigma bias b: sigma = |b| at every sample, b chosen so that A_c is about 0.9.  Q_c against the fp64
    definition over the call's own t_c.  The bar, 1e-3 of the coarse sample spacing, is derived: the device's weights carry a few fp32 ulp
    (1e-7 relative) of expf error each; theta and E are sums of them, so theta - E moves by about 1e-7 W; at A = 0.9 over at most 64 samples
    the weights fall by a factor 10 along the ray, so w_k >= W / 1000, and f = (theta - E) / w_k moves by under 1e-4 -- 1e-4 of a spacing,
    a tenth of the bar."""
    flags, B = MODES[mode]
    q = QSETS[3]
    row, col, pb, K = _inputs(oracle, B, dev, seed=7)
    near, far = pb[:, 15].double().cpu(), pb[:, 16].double().cpu()
    bias = float(2.3 / (far - near).mean())  # A = exp(-s) (1 - exp(-Nc s)) with Nc s = sigma (far - near): about 0.9
    p = oracle.make_weights(0)
    for k in p:
        p[k] = torch.zeros_like(p[k])
    p["network.sigma_layer.0.bias"] = torch.full_like(p["network.sigma_layer.0.bias"], bias)
    P = [v.to(dev).contiguous() for v in p.values()]
    rc, _, _, M, Q, _, ws = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, q=q)
    assert rc == 0
    view = lambda name, n: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, (B, n)).double().cpu()
    t_c, sig_c = view("t_c", Nc), view("sig_c", Nc)
    sigma = float(sig_c[0, 0])
    assert torch.equal(sig_c, torch.full_like(sig_c, sigma)) and abs(sigma - bias) <= 1e-2 * bias  # (bf16: the bias rounded)
    A = M[:, 1].cpu()
    print(f"constant field {mode} ({Nc}, {Nf}): sigma {sigma:.4f}, A_c in [{float(A.min()):.3f}, {float(A.max()):.3f}]")
    assert 0.6 < float(A.min()) and float(A.max()) < 0.995  # (at A < 0.999 the last weight is still above W / 1000)
    delta_c = ((far.float() - near.float()) / Nc).double()[:, None].expand(-1, Nc)  # quirk Q5, formed in fp32 as the kernel does
    ref = _definition_fp64(_weights_fp64(delta_c, torch.full_like(t_c, sigma)), t_c, q)
    spacing = ((far - near) / (Nc - 1)).numpy()[:, None]
    err = np.abs(Q[:, 0].double().cpu().numpy() - ref) / spacing
    print(f"constant field {mode} ({Nc}, {Nf}): worst |Q_c - fp64| = {err.max():.3e} of a coarse sample spacing (bar 1e-3)")
    assert err.max() <= 1e-3


def test_refusals_leave_the_sentinels(oracle, pkg, dev):
    _, P = _weights_dev(oracle, 4, True, dev)
    B, Nc, Nf = 8, 16, 32
    row, col, pb, K = _inputs(oracle, B, dev)
    ERR = -1
    nan = float("nan")
    cases = [dict(q=(0.5,), nq=0), dict(q=(0.5,), nq=5), dict(q=(0.5,), nq=-1), dict(q=(0.5,), null=("q",)), dict(q=(0.5,), null=("qdepth",)),
             dict(q=(0.5,), null=("maps",)), dict(q=(0.5, 0.0)), dict(q=(1.0,)), dict(q=(0.25, nan, 0.5)), dict(q=(-0.5,)), dict(q=(1.5,)),
             dict(q=(0.5,), flags=pkg._abi.SAVE_FOR_BACKWARD)]
    for kw in cases:
        flags = kw.pop("flags", 0)
        rc, Cc, Cf, M, Q, _, ws = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, sentinel=SENTINEL, **kw)
        torch.cuda.synchronize()
        assert rc == ERR, kw
        assert all(bool((x == SENTINEL).all()) for x in (Cc, Cf, M, Q)) and not bool(ws.any()), kw
    # the stage entries: the same checks (tests/test_quantile_cpu.py runs every one without a device); here the outputs stay untouched
    o, d = _coarse_operands(64, dev)
    for bad in ((0.0,), (0.5, 1.0), (nan,), ()):
        with pytest.raises(pkg._abi.NerfHipError):
            pkg.ops.coarse_composite_quantiles(d["t_c"], d["sig_c"], d["rgb_c"], o["near"], o["far"], o["delta0"], NF_COARSE, bad)
    m = _merge_operands(16, 32, dev)
    for bad in ((0.0,), (0.5, 1.0), (nan,), (0.1, 0.2, 0.3, 0.4, 0.5)):
        with pytest.raises(pkg._abi.NerfHipError):
            pkg.ops.merge_composite_quantiles(m["t_c"], m["t_f"], m["sig_c"], m["sig_f"], m["rgb_c"], m["rgb_f"], bad)
    rc, *_ = _call(pkg, P, row, col, pb, K, Nc, Nf, 0, q=(0.5,))  # and the good call goes through
    assert rc == 0


# ---------------------------------------------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16_pair"])
def test_render_quantiles_keep_the_batch_semantics(oracle, pkg, dev, mode):
    Bm, Nc, Nf = 400, 64, 128
    n = 5 * Bm + 1
    q = QSETS[3]
    row, col, pb, K, _ = oracle.fern_inputs(n, seed=12)
    p, _ = _weights_dev(oracle, 4, True, dev)
    m = pkg.NeRFModel(Nc, Nf, Bm)
    m.load_state_dict(p)
    m = m.to(dev)
    m.bf16_mlp = mode.startswith("bf16")
    rd, cd, pd = row.to(dev), col.to(dev), pb.float().to(dev)
    Cc0, Cf0, M0 = m.render(rd, cd, pd, K, maps=True)
    out = m.render(rd, cd, pd, K, maps=True, quantiles=q)
    assert len(out) == 4
    Cc, Cf, M, Q = out
    assert Q.shape == (n, 2, 3) and _same(Cc, Cc0) and _same(Cf, Cf0) and _same(M, M0)
    P = [v.detach() for v in m.network.parameters()]
    flags = pkg._abi.BF16_MLP if m.bf16_mlp else 0
    for s in range(0, n, Bm):
        e = min(s + Bm, n)
        r_, c_, p_ = rd[s:e], cd[s:e], pd[s:e]
        if e - s == 1:  # the library needs B >= 2: the ray twice, ray 0 = itself
            r_, c_, p_ = (torch.cat((x, x)) for x in (r_, c_, p_))
        rc, _, f, Mb, Qb, _, _ = _call(pkg, P, r_.contiguous(), c_.contiguous(), p_.contiguous(), K, Nc, Nf, flags, q=q)
        assert rc == 0 and _same(Q[s:e], Qb[: e - s]) and _same(M[s:e], Mb[: e - s]) and _same(Cf[s:e], f[: e - s]), s
    part = m.render(rd, cd, pd, K, lo=Bm - 3, hi=2 * Bm + 5, maps=True, quantiles=q)
    assert _same(part[3], Q[Bm - 3:2 * Bm + 5])
    with pytest.raises(ValueError, match="maps=True"):
        m.render(rd, cd, pd, K, quantiles=q)
    with pytest.raises(ValueError, match="quantiles="):
        m.render(rd, cd, pd, K, maps=True, quantiles=(0.5, 1.0))
    assert len(m.render(rd, cd, pd, K, maps=True, quantiles=None)) == 3


@pytest.fixture(scope="module")
def model(oracle, pkg, dev):
    g = load_golden("small_16_32")
    m = pkg.NeRFModel(int(g["Nc"]), int(g["Nf"]), 8)
    m.load_state_dict(oracle.make_weights(int(g["seed"]), bool(g["sharp"])))
    return m.to(dev)


LO, HI, RES, VH, VW = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 8, 16, 16


def _views(dev):
    poses = np.stack([TR.look_at((2.6, 0.3, 0.4), (0, 0, 0), near=1.0, far=4.5), TR.look_at((-0.5, -2.4, 1.0), (0, 0, 0), near=1.2, far=4.0)])
    return torch.from_numpy(np.array(poses)).to(dev), torch.from_numpy(TR.k_inv(VH, VW, 0.09)), VH, VW


def _by_hand(pkg, model, dev, views, col0, min_opacity, depth_stat, max_spread):
    """render(maps=True, quantiles=) per view, the depth-image rule written out here in torch, mesh.tsdf_integrate"""
    pb, K, H, W = views
    row = torch.arange(H, device=dev).repeat_interleave(W)
    col = torch.arange(W, device=dev).repeat(H)
    D, A, n_fg, n_rej = [], [], 0, 0
    for c in range(pb.shape[0]):
        _, _, M, Q = model.render(row, col, pb[c].expand(H * W, 17), K, maps=True, quantiles=(0.25, 0.5, 0.75))
        d, a, Q3 = M[:, col0], M[:, col0 + 1], Q[:, col0 // 2]
        fg = a >= min_opacity
        depth = torch.where(fg, Q3[:, 1] if depth_stat == "median" else d / a, torch.full_like(d, float("inf")))
        if max_spread is not None:
            rej = fg & (Q3[:, 2] - Q3[:, 0] > max_spread)
            depth = torch.where(rej, torch.full_like(d, float("nan")), depth)
            n_rej += int(rej.sum())
        n_fg += int(fg.sum())
        D.append(depth.view(H, W))
        A.append(a.view(H, W))
    D, A = torch.stack(D), torch.stack(A)
    lo32, hi32 = np.asarray(LO, F32), np.asarray(HI, F32)
    T, Wt = pkg.mesh.tsdf_volume(RES, dev)
    pkg.mesh.tsdf_integrate(T, Wt, lo32, pkg.nerf.grid_step(lo32, hi32, (RES,) * 3), D, pb, K, opacity=A, min_opacity=min_opacity)
    return T, Wt, A, D, n_fg, n_rej


def test_fuse_depth_median_and_spread(pkg, dev, model):
    views = _views(dev)
    A = _by_hand(pkg, model, dev, views, 0, 0.5, "mean", None)[2]
    mid = float(A.median())  # a threshold that leaves foreground and background pixels
    assert bool((A >= mid).any()) and bool((A < mid).any())
    # "mean" is today's path, bit for bit, and counts nothing
    old = model.fuse_depth(views, LO, HI, RES, min_opacity=mid)
    new = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, depth_stat="mean")
    assert _same(old[0], new[0]) and _same(old[1], new[1]) and model.last_tsdf_rejected == 0
    for kind, col0 in (("coarse", 0), ("fine", 2)):
        T, Wt, _, D, n_fg, _ = _by_hand(pkg, model, dev, views, col0, mid, "median", None)
        got = model.fuse_depth(views, LO, HI, RES, depth=kind, min_opacity=mid, depth_stat="median")
        one = model.fuse_depth(views, LO, HI, RES, depth=kind, min_opacity=mid, depth_stat="median", views_per_call=1)
        assert _same(got[0], T) and _same(got[1], Wt) and _same(one[0], T) and _same(one[1], Wt)
        assert int((Wt > 0).sum()) > 0 and n_fg > 0 and model.last_tsdf_rejected == 0
        # a spread threshold between the pixels' interquartile ranges rejects some of them, for either statistic
        _, _, Q = model.render(*_view_rays(views, 0, dev), maps=True, quantiles=(0.25, 0.5, 0.75))[1:]
        iqr = (Q[:, col0 // 2, 2] - Q[:, col0 // 2, 0])
        s = float(iqr.median())
        for stat in ("mean", "median"):
            T, Wt, _, D, n_fg, n_rej = _by_hand(pkg, model, dev, views, col0, mid, stat, s)
            got = model.fuse_depth(views, LO, HI, RES, depth=kind, min_opacity=mid, depth_stat=stat, max_spread=s)
            assert _same(got[0], T) and _same(got[1], Wt) and model.last_tsdf_rejected == n_rej and 0 < n_rej < n_fg
            assert int(torch.isnan(D).sum()) == n_rej
    assert not _same(model.fuse_depth(views, LO, HI, RES, min_opacity=mid, depth_stat="median")[0], old[0])  # the statistic matters
    with pytest.raises(ValueError, match="depth_stat="):
        model.fuse_depth(views, LO, HI, RES, depth_stat="mode")
    with pytest.raises(ValueError, match="max_spread="):
        model.fuse_depth(views, LO, HI, RES, max_spread=-1.0)


def _view_rays(views, c, dev):
    pb, K, H, W = views
    return torch.arange(H, device=dev).repeat_interleave(W), torch.arange(W, device=dev).repeat(H), pb[c].expand(H * W, 17), K


def test_max_spread_zero_rejects_every_foreground_pixel(pkg, dev, model):
    views = _views(dev)
    A = _by_hand(pkg, model, dev, views, 0, 0.5, "mean", None)[2]
    mid = float(A.median())
    T, Wt, A, D, n_fg, n_rej = _by_hand(pkg, model, dev, views, 0, mid, "median", 0.0)
    assert n_rej == n_fg == int((A >= mid).sum()) > 0  # (every foreground ray's weight is spread over more than one sample: IQR > 0)
    got = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, depth_stat="median", max_spread=0.0)
    assert model.last_tsdf_rejected == n_fg and _same(got[0], T) and _same(got[1], Wt)
    # only carving observations are left: every observed voxel holds exactly T = 1 (val = 1 each time), and without carving nothing is observed
    assert int((got[1] > 0).sum()) > 0 and bool((got[0][got[1] > 0] == 1.0).all()) and bool((got[0][got[1] == 0] == 0.0).all())
    none = model.fuse_depth(views, LO, HI, RES, min_opacity=mid, depth_stat="median", max_spread=0.0, carve=False)
    assert not bool(none[1].any()) and not bool(none[0].any())
    mesh = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, depth_stat="median", max_spread=float("inf"), color=False)
    ref = model.extract_mesh_tsdf(views, LO, HI, RES, min_opacity=mid, depth_stat="median", color=False)
    assert model.last_tsdf_rejected == 0 and torch.equal(mesh.verts, ref.verts) and torch.equal(mesh.faces, ref.faces)


def test_runner_tsdf_depth_stat(pkg, dev, tmp_path, capsys):
    import glob

    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    tsdf_line = lambda: [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[MESH]") and "[TSDF]" in ln]
    capsys.readouterr()
    run.extract_mesh(16, 1.0, save=True, tsdf_from="train", tsdf_every=2)
    plain = tsdf_line()
    assert len(plain) == 1 and "depth," not in plain[0] and "rejected" not in plain[0]
    got = run.extract_mesh(16, 1.0, save=True, tsdf_from="train", tsdf_every=2, tsdf_depth_stat="median", tsdf_max_spread=0.2)
    line = tsdf_line()
    files = glob.glob(rs + "*_mesh16_tsdf_median.ply")
    assert len(line) == 1 and len(files) == 1 and len(glob.glob(rs + "*_mesh16_tsdf.ply")) == 1
    assert f", median depth, {run.model.last_tsdf_rejected} pixels rejected (depth spread > 0.2)" in line[0]
    views = (run.train_rays.poses[::2], run.K_inv, 24, 24)
    want = run.model.extract_mesh_tsdf(views, (-1.5,) * 3, (1.5,) * 3, 16, depth_stat="median", max_spread=0.2)
    assert np.array_equal(got.verts, want.verts.cpu().numpy()) and np.array_equal(got.faces, want.faces.cpu().numpy())
    # the spread alone: the mean is fused, the line says so, the name stays
    run.extract_mesh(16, 1.0, save=False, tsdf_from="train", tsdf_every=2, tsdf_max_spread=0.2)
    assert ", mean depth, " in tsdf_line()[0]
    # without the options: the line of before
    run.extract_mesh(16, 1.0, save=False, tsdf_from="train", tsdf_every=2)
    assert tsdf_line() == plain
    with pytest.raises(ValueError, match="tsdf_depth_stat"):
        run.extract_mesh(16, 1.0, save=False, tsdf_from="val", tsdf_depth_stat="mode")
