"""GPU: per-ray normal maps (rule NM of include/nerf_hip.h) -- k_normal_composite through its stage entry, the whole
nerf_hip_forward_normals call, NeRFModel.render(maps=True, normals=), NeRFRunner.display(normals=True) and the normal preview.

  * every output the normals call shares with the maps call has that call's bits, the main workspace's t_c / w_c / t_f included;
  * N against the numpy restatement (tests/normal_reference.py) evaluated on the call's OWN operands -- its weights and depths from the two
    workspaces, the points nerf_hip_field forms at those depths, the gradients nerf_hip_query_grad gives at those points -- inside
    |N - fp32(S64)| <= ulp32(|S64|) + 1e-12 sum |w_i| per component: one fp32 rounding plus a possible tie, and the reordering of at most
    2,048 fp64 terms (below 2048 * 2^-53 sum |w_i| = 2.3e-13 sum |w_i|, with a 4x margin).  Both terms are derived, none measured;
  * a constant field gives N = 0 exactly, a field sigma = |sin(f_0 x)| gives N along x with the sign sum of the call's own samples;
  * the Python layers keep render's batch semantics.
"""
import ctypes
import struct
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

import normal_reference as NR

pytestmark = pytest.mark.gpu
F32 = np.float32
SENTINEL = -7.0
CHUNK = 256 * 4 * 32 * 4  # kernels.h QGRAD_CHUNK


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _within(N, w, g):
    """N [B, 3] (device or CPU tensor) against the restatement on w [B, n], g [B, n, 3] -> (worst excess over the bound, S64)"""
    w, g = w.cpu().numpy(), g.cpu().numpy()
    S = NR.composite64(w, g)
    err = np.abs(N.cpu().numpy().astype(np.float64) - S.astype(F32).astype(np.float64))
    return float((err - NR.bound(w, S)).max()), S


# ---------------------------------------------------------------------------------------------------------------
# 1. the stage
# ---------------------------------------------------------------------------------------------------------------
B_STAGE = 7  # 7 rays: the second workgroup of four waves has one wave behind the batch


def _stage_operands(N, dev):
    gen = torch.Generator().manual_seed(N)
    w = torch.rand(B_STAGE, N, generator=gen)
    g = torch.randn(B_STAGE, N, 3, generator=gen) * torch.exp(4.0 * torch.randn(B_STAGE, N, 1, generator=gen))
    inf, nan = float("inf"), float("nan")
    salt = [(0.0, 0.0, 0.0), (inf, 1.0, 2.0), (1.0, -inf, 0.0), (nan, 1.0, 1.0), (3e38, 3e38, 0.0)]
    for r in range(B_STAGE):  # every ray carries the salted samples its length has room for
        for k, v in enumerate(salt):
            i = (5 * r + 11 * k) % N
            if N > 2 * len(salt) or (r, k) == (1, 0):
                g[r, i] = torch.tensor(v)
        if N > 4:
            w[r, (3 * r + 1) % N] = 0.0
            w[r, (3 * r + 2) % N] = nan
    if N <= 2:
        w[2, 0], w[3, N - 1] = 0.0, nan
    return w.to(dev).contiguous(), g.to(dev).contiguous()


@pytest.mark.parametrize("stride", [3, 6])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 200, 2048])
def test_stage(pkg, dev, N, stride):
    w, g = _stage_operands(N, dev)
    out = pkg.ops.normal_composite(w, g, out_stride=stride, sentinel=SENTINEL)
    assert out.shape == (B_STAGE, stride) and bool(torch.isfinite(out).all())
    if stride > 3:
        assert bool((out[:, 3:] == SENTINEL).all())  # nothing but the three components is written
    excess, S = _within(out[:, :3], w, g)
    print(f"stage N={N} stride={stride}: worst |N - fp32(S64)| - bound = {excess:.3e}, max |S64| = {np.abs(S).max():.3e}")
    assert excess <= 0.0
    again = pkg.ops.normal_composite(w, g, out_stride=stride, sentinel=SENTINEL)
    assert _same(out, again)  # identical bits run to run
    five = pkg.ops.normal_composite(w, g, out_stride=stride, sentinel=SENTINEL, rays=5)  # the rays behind the batch store nothing
    assert _same(five[:5], out[:5]) and bool((five[5:] == SENTINEL).all())
    A = torch.nan_to_num(w, nan=0.0).double().sum(1)
    assert bool((out[:, :3].double().norm(dim=1) <= A * (1 + 1e-6)).all())


def test_stage_refusals_leave_the_output(pkg, dev):
    w, g = _stage_operands(64, dev)
    out = torch.full((B_STAGE, 3), SENTINEL, device=dev)
    L = pkg._abi.lib()
    for B, N, stride in ((-1, 64, 3), (B_STAGE, 0, 3), (B_STAGE, 2049, 3), (B_STAGE, 64, 2)):
        assert L.nerf_hip_normal_composite(w.data_ptr(), g.data_ptr(), B, N, out.data_ptr(), stride, None) == -1
    assert L.nerf_hip_normal_composite(w.data_ptr(), g.data_ptr(), 0, 64, out.data_ptr(), 3, None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


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


def _weights_dev(oracle, seed, sharp, dev):
    p = oracle.make_weights(seed, sharp)
    return p, [v.to(dev).contiguous() for v in p.values()]


def _inputs(oracle, B, dev, seed=3):
    row, col, pb, K, _ = oracle.fern_inputs(B, seed=seed)  # per-image near / far
    return row.to(dev).contiguous(), col.to(dev).contiguous(), pb.float().to(dev).contiguous(), K


def _maps_call(pkg, P, row, col, pb, K, Nc, Nf, flags):
    """one direct nerf_hip_forward_maps call on a fresh workspace -> (C_c, C_f, maps, status, ws)"""
    _abi = pkg._abi
    dev, B = P[0].device, row.shape[0]
    n = _abi.ws_bytes(B, Nc, Nf, flags)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    Cc, Cf, M = (torch.empty(B, k, device=dev) for k in (3, 3, 4))
    stream = torch.cuda.current_stream(dev).cuda_stream
    _abi.check(_abi.lib().nerf_hip_forward_maps(_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(),
                                                _abi.f32_array(K.reshape(-1).tolist()), None, B, Nc, Nf, pkg.nerf.LAST_DELTA, Cc.data_ptr(),
                                                Cf.data_ptr(), M.data_ptr(), ws.data_ptr(), n, flags, stream))
    return Cc, Cf, M, _status(pkg, ws), ws


def _status(pkg, ws):
    st = ctypes.c_uint32(0)
    pkg._abi.check(pkg._abi.lib().nerf_hip_read_status(ws.data_ptr(), ws.numel(), ctypes.byref(st), torch.cuda.current_stream(ws.device).cuda_stream))
    return int(st.value)


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("mode", list(MODES))
def test_shared_outputs_are_the_maps_calls(oracle, pkg, dev, mode, Nc, Nf):
    flags, B = MODES[mode]
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K = _inputs(oracle, B, dev)
    c0, f0, M0, s0, ws0 = _maps_call(pkg, P, row, col, pb, K, Nc, Nf, flags)
    c, f, M, Nrm, ws, nws = pkg.ops.forward_normals(P, row, col, pb, K, Nc, Nf, flags=flags, passes=3, sentinel=SENTINEL)
    assert _same(c, c0) and _same(f, f0) and _same(M, M0) and _status(pkg, ws) == s0
    for name, n in (("t_c", Nc), ("w_c", Nc), ("t_f", Nf)):
        v0, v = (pkg._abi.ws_view(x, B, Nc, Nf, flags, name, (B, n)) for x in (ws0, ws))
        assert _same(v, v0), name
    assert ws.numel() == ws0.numel()
    assert bool(torch.isfinite(Nrm).all()) and not bool((Nrm == SENTINEL).any())
    assert bool((Nrm[:, 0].double().norm(dim=1) <= M[:, 1].double() * (1 + 1e-6)).all())
    assert bool((Nrm[:, 1].double().norm(dim=1) <= M[:, 3].double() * (1 + 1e-6)).all())
    for passes, kept in ((1, 1), (2, 0)):  # one pass alone: its row has the bits of the call for both, the other row is untouched
        c1, f1, M1, N1, ws1, _ = pkg.ops.forward_normals(P, row, col, pb, K, Nc, Nf, flags=flags, passes=passes, sentinel=SENTINEL, nws=nws)
        assert _same(c1, c0) and _same(f1, f0) and _same(M1, M0)
        assert _same(N1[:, 1 - kept], Nrm[:, 1 - kept]) and bool((N1[:, kept] == SENTINEL).all())


OPERAND_CASES = [(7, 64, 128), (7, 16, 32), (7, 24, 40), (7, 65, 63), (2, 64, 128), (700, 64, 128)]


def _own_operands(pkg, P, row, col, pb, K, B, Nc, Nf, flags, ws, nws):
    """the call's own (w, t) of both passes from the two workspaces, the points nerf_hip_field forms at those depths and
    nerf_hip_query_grad's gradients at those points -> {pass: (w, t, pts, g)}"""
    N = Nc + Nf
    view = lambda name, n: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, (B, n))
    bundle = pkg._abi.normals_ws_view(nws, B, Nc, Nf, "bundle", (B, N, 5))
    out = {}
    for name, w, t in (("coarse", view("w_c", Nc), view("t_c", Nc)),
                       ("fine", pkg._abi.normals_ws_view(nws, B, Nc, Nf, "w_m", (B, N)), bundle[:, :, 0].contiguous())):
        pts = pkg.ops.field(P, row, col, pb, K, t, debug=True)[2]
        g = pkg.ops.query_grad(P, pts.reshape(-1, 3))[2].view(B, -1, 3)
        out[name] = (w.clone(), t.clone(), pts, g)
    return out


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,Nc,Nf", OPERAND_CASES)
def test_against_the_restatement_on_the_calls_own_operands(oracle, pkg, dev, B, Nc, Nf, mode, sharp):
    flags = pkg._abi.BF16_MLP if mode == "bf16" else 0
    _, P = _weights_dev(oracle, 4, sharp, dev)
    row, col, pb, K = _inputs(oracle, B, dev, seed=5)
    c, f, M, Nrm, ws, nws = pkg.ops.forward_normals(P, row, col, pb, K, Nc, Nf, flags=flags, passes=3, sentinel=SENTINEL)
    own = _own_operands(pkg, P, row, col, pb, K, B, Nc, Nf, flags, ws, nws)
    N = Nc + Nf
    # the chunk still resident in the side workspace: the last chunk of whole rays of the fine pass
    per = CHUNK // N
    r0 = (B - 1) // per * per
    if B == 700:
        assert B * N > CHUNK and r0 == 682  # more than one chunk, and 131,072 / 192 is no whole number of rays
    n_res = (B - r0) * N
    w_f, t_f, pts_f, g_f = own["fine"]
    assert _same(pkg._abi.normals_ws_view(nws, B, Nc, Nf, "points", (CHUNK, 3))[:n_res], pts_f[r0:].reshape(-1, 3))
    assert _same(pkg._abi.normals_ws_view(nws, B, Nc, Nf, "grad", (CHUNK, 3))[:n_res], g_f[r0:].reshape(-1, 3))
    for p, name in enumerate(("coarse", "fine")):
        w, t, pts, g = own[name]
        excess, S = _within(Nrm[:, p], w, g)
        print(f"{mode} sharp={sharp} B={B} ({Nc}, {Nf}) {name}: worst |N - fp32(S64)| - bound = {excess:.3e}, max |N| = {np.abs(S).max():.3e}")
        assert excess <= 0.0
        A = M[:, 2 * p + 1].double()
        assert bool((Nrm[:, p].double().norm(dim=1) <= A * (1 + 1e-6)).all())
    assert float(Nrm.abs().max()) > 0.0  # (a field with gradients: the normals are not all zero)


def test_constant_field_has_no_normal(oracle, pkg, dev):
    """every weight zero and the sigma bias b: sigma = |b| everywhere, every g_i is 0, so N is exactly 0 while A is not"""
    B, Nc, Nf = 64, 64, 128
    row, col, pb, K = _inputs(oracle, B, dev, seed=7)
    bias = float(2.3 / (pb[:, 16] - pb[:, 15]).double().mean())
    p = oracle.make_weights(0)
    for k in p:
        p[k] = torch.zeros_like(p[k])
    p["network.sigma_layer.0.bias"] = torch.full_like(p["network.sigma_layer.0.bias"], bias)
    P = [v.to(dev).contiguous() for v in p.values()]
    for flags in (0, pkg._abi.BF16_MLP):
        _, _, M, Nrm, _, nws = pkg.ops.forward_normals(P, row, col, pb, K, Nc, Nf, flags=flags, passes=3, sentinel=SENTINEL)
        assert bool((Nrm == 0).all())
        assert float(M[:, 1].min()) > 0.5 and float(M[:, 3].min()) > 0.5
        assert not bool(pkg._abi.normals_ws_view(nws, B, Nc, Nf, "grad", (CHUNK, 3))[: B * (Nc + Nf)].any())


def _sine_weights(oracle):
    """sigma = |sin(f_0 x)| (tests/test_gpu_query_grad.py's field): h_0[0] = relu(gamma_p[0] + 2) = sin(phi) + 2 carried through layers
    1..7 by unit weights, w_sigma[0] = 1, b_sigma = -2; every other weight 0."""
    w = OrderedDict((k, torch.zeros(s)) for k, s in oracle.PARAM_SHAPES.items())
    w["network.point_layer.0.0.weight"][0, 0] = 1.0
    w["network.point_layer.0.0.bias"][0] = 2.0
    for i in range(1, 8):
        w[f"network.point_layer.{i}.0.weight"][0, 0] = 1.0
    w["network.sigma_layer.0.weight"][0, 0] = 1.0
    w["network.sigma_layer.0.bias"][0] = -2.0
    return w


def test_sine_field_normals_point_along_x(oracle, pkg, dev):
    """sigma = |sin(f_0 x)|: d sigma / dx = sign(sin) f_0 cos, nothing along y and z, so every n_i is within 1e-6 of (+-1, 0, 0) -- the bar
    tests/test_gpu_query_grad.py measured for this field's normals -- and N_x = -sum_i w_i sign(d sigma / dx at p_i) to 1e-6 A over the call's
    own weights and points.  A sample within 1e-5 rad of a zero of sin or cos (where fp32 decides the sign, or the gradient is 0) may
    land on either side: its weight is added to that ray's allowance."""
    B, Nc, Nf = 64, 64, 128
    P = [v.to(dev).contiguous() for v in _sine_weights(oracle).values()]
    row, col, pb, K = _inputs(oracle, B, dev, seed=9)
    f0 = oracle.frequencies()[0][0]
    _, _, M, Nrm, ws, nws = pkg.ops.forward_normals(P, row, col, pb, K, Nc, Nf, passes=3, sentinel=SENTINEL)
    own = _own_operands(pkg, P, row, col, pb, K, B, Nc, Nf, 0, ws, nws)
    for p, name in enumerate(("coarse", "fine")):
        w, t, pts, g = own[name]
        A = M[:, 2 * p + 1].double().cpu()
        assert float(A.min()) > 0.3
        N = Nrm[:, p].double().cpu()
        assert bool((N[:, 1:].abs() <= 1e-6 * A[:, None]).all())
        phi = (pts[:, :, 0].cpu() * f0).double()  # fp32(x * f_0), as the encoding forms it
        s, c = torch.sin(phi), torch.cos(phi)
        unsure = (s.abs() < 1e-5) | (c.abs() < 1e-5)
        wd = w.double().cpu()
        want = -(wd * torch.sign(s) * torch.sign(c) * (~unsure)).sum(1)
        slack = (wd * unsure).sum(1)
        err = (N[:, 0] - want).abs()
        print(f"sine field {name}: worst |N_x - want| / A = {float((err / A).max()):.3e}, unsure samples {int(unsure.sum())}, "
              f"|N| / A in [{float((N.norm(dim=1) / A).min()):.3f}, {float((N.norm(dim=1) / A).max()):.3f}]")
        assert bool((err <= 1e-6 * A + slack).all())
        assert float(N[:, 0].abs().max()) > 0.05  # (the sign sum does not vanish on every ray)


def test_refusals_leave_the_outputs(oracle, pkg, dev):
    _, P = _weights_dev(oracle, 4, True, dev)
    B, Nc, Nf = 8, 16, 32
    row, col, pb, K = _inputs(oracle, B, dev)
    _abi = pkg._abi
    ws = torch.zeros(_abi.ws_bytes(B, Nc, Nf, 0), dtype=torch.uint8, device=dev)
    need = _abi.normals_ws_bytes(B, Nc, Nf)
    nws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    Cc, Cf, M, Nrm = (torch.full(s, SENTINEL, device=dev) for s in ((B, 3), (B, 3), (B, 4), (B, 2, 3)))
    K9 = _abi.f32_array(K.reshape(-1).tolist())

    def call(passes=2, normals=Nrm.data_ptr(), nptr=nws.data_ptr(), nbytes=need, maps=M.data_ptr(), flags=0):
        return _abi.lib().nerf_hip_forward_normals(_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, None, B, Nc, Nf, 1e-4,
                                                   Cc.data_ptr(), Cf.data_ptr(), maps, ws.data_ptr(), ws.numel(), flags, None, passes, normals,
                                                   nptr, nbytes)

    for kw in (dict(passes=0), dict(passes=4), dict(normals=None), dict(nptr=None), dict(maps=None), dict(nbytes=need - 1),
               dict(nptr=nws.data_ptr() + 128), dict(flags=_abi.SAVE_FOR_BACKWARD)):
        assert call(**kw) == -1, kw
        torch.cuda.synchronize()
        assert all(bool((x == SENTINEL).all()) for x in (Cc, Cf, M, Nrm)) and not bool(ws.any()) and not bool(nws.any()), kw
    assert call() == 0  # and the good call goes through
    torch.cuda.synchronize()
    assert bool((Nrm[:, 0] == SENTINEL).all()) and bool(torch.isfinite(Nrm[:, 1]).all())


# ---------------------------------------------------------------------------------------------------------------
# Python
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16_pair"])
def test_render_normals_keep_the_batch_semantics(oracle, pkg, dev, mode):
    Bm, Nc, Nf = 400, 64, 128
    n = 3 * Bm + 1  # three batches (their images, so their near / far, differ) and a one-ray tail
    row, col, pb, K, _ = oracle.fern_inputs(n, seed=12)
    assert len({(float(a), float(b)) for a, b in pb[::Bm, 15:17]}) > 1  # batches with different near / far
    p, _ = _weights_dev(oracle, 4, True, dev)
    m = pkg.NeRFModel(Nc, Nf, Bm)
    m.load_state_dict(p)
    m = m.to(dev)
    m.bf16_mlp = mode.startswith("bf16")
    rd, cd, pd = row.to(dev), col.to(dev), pb.float().to(dev)
    Cc0, Cf0, M0 = m.render(rd, cd, pd, K, maps=True)
    out = m.render(rd, cd, pd, K, maps=True, normals="both")
    assert len(out) == 4
    Cc, Cf, M, Nrm = out
    assert Nrm.shape == (n, 2, 3) and _same(Cc, Cc0) and _same(Cf, Cf0) and _same(M, M0) and bool(torch.isfinite(Nrm).all())
    P = [v.detach() for v in m.network.parameters()]
    flags = pkg._abi.BF16_MLP if m.bf16_mlp else 0
    for s in range(0, n, Bm):
        e = min(s + Bm, n)
        r_, c_, p_ = rd[s:e], cd[s:e], pd[s:e]
        if e - s == 1:  # the library needs B >= 2: the ray twice, ray 0 = itself
            r_, c_, p_ = (torch.cat((x, x)) for x in (r_, c_, p_))
        _, fb, Mb, Nb, _, _ = pkg.ops.forward_normals(P, r_.contiguous(), c_.contiguous(), p_.contiguous(), K, Nc, Nf, flags=flags, passes=3)
        assert _same(Nrm[s:e], Nb[: e - s]) and _same(M[s:e], Mb[: e - s]) and _same(Cf[s:e], fb[: e - s]), s
    part = m.render(rd, cd, pd, K, lo=Bm - 3, hi=2 * Bm + 5, maps=True, normals="both")
    assert _same(part[3], Nrm[Bm - 3:2 * Bm + 5])
    # the rows asked for, NaN elsewhere; True = "fine"
    fine = m.render(rd, cd, pd, K, maps=True, normals=True)[3]
    assert _same(fine[:, 1], Nrm[:, 1]) and bool(torch.isnan(fine[:, 0]).all())
    assert _same(m.render(rd, cd, pd, K, maps=True, normals="fine")[3][:, 1], Nrm[:, 1])
    coarse = m.render(rd, cd, pd, K, maps=True, normals="coarse")[3]
    assert _same(coarse[:, 0], Nrm[:, 0]) and bool(torch.isnan(coarse[:, 1]).all())
    # behind Q when quantiles are asked for too
    q = (0.25, 0.5, 0.75)
    Q0 = m.render(rd, cd, pd, K, maps=True, quantiles=q)[3]
    both = m.render(rd, cd, pd, K, maps=True, quantiles=q, normals="both")
    assert len(both) == 5 and _same(both[3], Q0) and _same(both[4], Nrm) and _same(both[2], M0) and _same(both[1], Cf0)
    # normals=False is the call of before
    plain = m.render(rd, cd, pd, K, maps=True, normals=False)
    assert len(plain) == 3 and _same(plain[2], M0) and _same(plain[1], Cf0)
    assert len(m.render(rd, cd, pd, K, normals=False)) == 2
    with pytest.raises(ValueError, match="maps=True"):
        m.render(rd, cd, pd, K, normals=True)
    with pytest.raises(ValueError, match="normals="):
        m.render(rd, cd, pd, K, maps=True, normals="all")
    assert len(m.render(rd, cd, pd, K, lo=5, hi=5, maps=True, normals=True)) == 4  # an empty range keeps the tuple's shape
    # the multi-rank path's shards (no collective in the data path: both ranks' calls from this process) put the fine row together
    import importlib

    par = importlib.import_module("nerf_tiny_amd.parallel")
    shards = [par.render_rows_sharded(m, rd, cd, pd, K, r, 2, maps=True, normals=True) for r in range(2)]
    assert [len(s) for s in shards] == [5, 5] and shards[0][0] == 0 and shards[0][1] == shards[1][0] and shards[1][1] == n
    assert _same(torch.cat([s[4] for s in shards]), Nrm[:, 1]) and _same(torch.cat([s[3] for s in shards]), M0)
    with pytest.raises(ValueError, match="maps=True"):
        par.render_rows_sharded(m, rd, cd, pd, K, 0, 2, normals=True)


def _png(path):
    """the 8-bit RGB PNG mesh.png_bytes writes (one IDAT, filter 0 on every row) -> [H, W, 3] uint8"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, shape = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            W, H, depth, kind = struct.unpack(">IIBB", body[:10])
            assert (depth, kind) == (8, 2)
            shape = (H, W)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(shape[0], shape[1], 3)


def test_display_normals_and_the_preview(pkg, dev, tmp_path):
    import os

    H = W = 24
    scene = pkg.data.synthetic_scene(n_pic=2, H=H, W=W, seed=4)
    rs = str(tmp_path) + "/res/"
    kw = dict(gpu=0, img_dir="", results_path=rs, ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256, learning=1e-3,
              lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1)
    torch.manual_seed(0)
    run = pkg.NeRFRunner(continue_=False, **kw)
    frames0, depth0, acc0 = run.display(save=False, maps=True)
    out = run.display(save=True, maps=True, normals=True)
    assert len(out) == 4
    frames, depth, acc, nrm = out
    assert np.array_equal(frames, frames0) and np.array_equal(depth, depth0, equal_nan=True) and np.array_equal(acc, acc0)
    assert nrm.shape == (2, H, W, 3) and nrm.dtype == np.float32 and np.isfinite(nrm).all()
    # against render: the display batches in pixel order, the tail < batch_ray left out (white frame, zero normal)
    rays = run.disp_rays
    n_keep = rays.num_pix // 256 * 256
    row, col, _, pb, pic = rays.gather(torch.arange(n_keep, device=dev))
    prev = run.model.batch_ray
    run.model.batch_ray = 256
    try:
        Nrm = run.model.render(row, col, pb, run.K_inv, maps=True, normals="fine")[3]
    finally:
        run.model.batch_ray = prev
    want = np.zeros((2, H, W, 3), np.float32)
    want[pic.cpu().numpy(), row.cpu().numpy(), col.cpu().numpy()] = Nrm[:, 1].cpu().numpy()
    assert np.array_equal(nrm, want) and np.abs(nrm).max() > 0
    assert n_keep < rays.num_pix  # (the tail's pixels: the zeros of `want`)
    # the preview beside the frames: 0.5 + 0.5 * the unit normal, mid grey where there is none
    save_dir = rs + run.start_time + "/"
    for i in range(2):
        path = save_dir + f"{i}_normal.png"
        assert os.path.exists(path)
        img = _png(path)
        assert img.shape == (H, W, 3)
        unit = pkg.nerf.unit_normals(nrm[i], acc[i])
        assert np.array_equal(img, np.rint((0.5 + 0.5 * unit).clip(0, 1) * 255.0).astype(np.uint8))
        bg = ~((acc[i] >= 0.5) & (np.abs(nrm[i]).sum(-1) > 0))
        assert bg.any() and (img[bg] == 128).all()
    with pytest.raises(ValueError, match="maps=True"):
        run.display(save=False, normals=True)
    assert len(run.display(save=False, maps=True)) == 3  # without the keyword: the tuple of before
