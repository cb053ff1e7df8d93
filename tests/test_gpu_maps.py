"""GPU: nerf_hip_forward_maps -- each ray's expected depth and accumulated opacity beside the colours, maps[B][4] = (D_c, A_c, D_f, A_f):

  * the colours and the status word are nerf_hip_forward's, bit for bit, in every inference mode (the bf16 ray-pair sizes included);
  * the coarse maps are the fp64 sums over the call's own w_c / t_c (workspace) to fp32 summation order;
  * the fine maps follow the oracle's restatement (sum w t_s, sum w over the merged, sorted samples) at the colours' bars;
  * a constant field (every weight zero, sigma = |bias|) gives the fp64 evaluation of the definition over the call's own sample depths;
  * NeRFModel.render(maps=True) keeps the batch semantics of render(), NeRFRunner.display(maps=True) writes its files and keeps its frames.
"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_inputs, load_golden, max_rel

pytestmark = pytest.mark.gpu

MODES = {  # name -> (flags, rays)
    "fp32": (0, 256),
    "tile": (1 << 1, 256),
    "split": (1 << 4, 256),
    "bf16_pair": (1 << 2, 256),    # at (64, 128) the one-launch ray-pair kernel for nerf_hip_forward, separate launches for the maps call
    "bf16_large": (1 << 2, 1024),  # beyond the pair kernel's sizes: separate launches for both
    "corrected": (1 << 5, 256),
}
SAMPLES = [(64, 128), (16, 32), (24, 40)]  # the shipped counts, small_16_32's, and a merged count that is no power of two (P = 64 > 64 samples)


def _weights_dev(oracle, seed, sharp, dev):
    p = oracle.make_weights(seed, sharp)
    return p, [v.to(dev).contiguous() for v in p.values()]


def _call(pkg, P, row, col, pb, K, Nc, Nf, flags, maps):
    """One direct nerf_hip_forward(_maps) call on a fresh workspace -> (C_c, C_f, maps or None, status, ws)."""
    _abi = pkg._abi
    dev = P[0].device
    B = row.shape[0]
    n = _abi.ws_bytes(B, Nc, Nf, flags)
    ws = torch.zeros(n, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    Cc = torch.full((B, 3), float("nan"), device=dev)
    Cf = torch.full((B, 3), float("nan"), device=dev)
    K9 = _abi.f32_array(K.reshape(-1).tolist())
    args = (_abi.ptr_array(P), row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, None, B, Nc, Nf, pkg.nerf.LAST_DELTA, Cc.data_ptr(), Cf.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    M = None
    if maps:
        M = torch.full((B, 4), float("nan"), device=dev)
        _abi.check(_abi.lib().nerf_hip_forward_maps(*args, M.data_ptr(), ws.data_ptr(), n, flags, stream))
    else:
        _abi.check(_abi.lib().nerf_hip_forward(*args, ws.data_ptr(), n, flags, stream))
    st = ctypes.c_uint32(0)
    _abi.check(_abi.lib().nerf_hip_read_status(ws.data_ptr(), n, ctypes.byref(st), stream))
    return Cc, Cf, M, int(st.value), ws


def _inputs(oracle, B, dev, seed=3):
    row, col, pb, K, _ = oracle.fern_inputs(B, seed=seed)  # per-image near / far
    return row.to(dev).contiguous(), col.to(dev).contiguous(), pb.float().to(dev).contiguous(), K


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("mode", list(MODES))
def test_colours_and_status_unchanged(oracle, pkg, dev, mode, Nc, Nf):
    flags, B = MODES[mode]
    _, P = _weights_dev(oracle, 4, True, dev)
    row, col, pb, K = _inputs(oracle, B, dev)
    c0, f0, _, s0, _ = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, False)
    c1, f1, M, s1, _ = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, True)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and torch.equal(f0, f1)
    assert s0 == s1
    assert torch.isfinite(M).all()
    A = M[:, 1::2]
    assert float(A.min()) >= 0.0 and float(A.max()) <= 1.0 + 1e-6


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("mode", ["fp32", "split", "bf16_pair", "corrected"])
def test_coarse_maps_are_the_sums_of_the_calls_own_weights(oracle, pkg, dev, mode, Nc, Nf):
    flags, B = MODES[mode]
    _, P = _weights_dev(oracle, 1, False, dev)
    row, col, pb, K = _inputs(oracle, B, dev, seed=5)
    _, _, M, _, ws = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, True)
    w_c = pkg._abi.ws_view(ws, B, Nc, Nf, flags, "w_c", (B, Nc)).double().cpu()
    t_c = pkg._abi.ws_view(ws, B, Nc, Nf, flags, "t_c", (B, Nc)).double().cpu()
    M = M.double().cpu()
    D, A = (w_c * t_c).sum(1), w_c.sum(1)
    assert float(((M[:, 0] - D).abs() / D.abs().clamp_min(1e-20)).max()) <= 1e-6
    assert float((M[:, 1] - A).abs().max()) <= 1e-6


GOLDEN = ["cfg1_lego_crop32", "cfg1_lego_crop32_sharp", "cfg4_fern_rand512", "small_16_32"]


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("mode", ["fp32", "tile", "split", "bf16_large", "corrected"])
def test_maps_against_the_oracle(oracle, pkg, dev, mode, name):
    """fp64 sums over the oracle's own weights and (sorted) depths.  Bars: the colours' -- 1e-4 max-rel for the fp32 kinds; for the bf16
    MLP against its emulation the bars tests/test_gpu_bf16.py holds C_coarse / C_fine to (5e-3 / 3e-2)."""
    flags = MODES[mode][0]
    g = load_golden(name)
    row, col, pb, K, _ = golden_inputs(g)
    Nc, Nf = int(g["Nc"]), int(g["Nf"])
    p, P = _weights_dev(oracle, int(g["seed"]), bool(g["sharp"]), dev)
    st = {}
    kw = dict(mlp=oracle.mlp_bf16, check=False) if mode.startswith("bf16") else dict(corrected=(mode == "corrected"))
    with torch.no_grad():
        oracle.render(p, row, col, pb, K, Nc, Nf, stages=st, **kw)
    d = lambda x: x.contiguous().to(dev)
    _, _, M, _, _ = _call(pkg, P, d(row), d(col), d(pb.float()), K, Nc, Nf, flags, True)
    M = M.double().cpu()
    w_c, t_c, w, t_s = (st[k].double() for k in ("w_c", "t_c", "w", "t_s"))
    ref = torch.stack(((w_c * t_c).sum(1), w_c.sum(1), (w * t_s).sum(1), w.sum(1)), 1)
    bc, bf = (5e-3, 3e-2) if mode.startswith("bf16") else (1e-4, 1e-4)
    assert max_rel(M[:, 0], ref[:, 0]) < bc and max_rel(M[:, 1], ref[:, 1]) < bc
    assert max_rel(M[:, 2], ref[:, 2]) < bf and max_rel(M[:, 3], ref[:, 3]) < bf


def _weights_fp64(delta, sigma):
    """the definition in fp64: s = delta sigma, T_i = exp(-sum_{j <= i} s_j) (inclusive, as the reference), w = T (1 - exp(-s))."""
    s = delta * sigma
    return torch.exp(-torch.cumsum(s, 1)) * (1.0 - torch.exp(-s))


@pytest.mark.parametrize("Nc,Nf", SAMPLES)
@pytest.mark.parametrize("bias", [0.5, -3.0])
@pytest.mark.parametrize("mode", ["fp32", "split", "bf16_large", "corrected"])
def test_constant_field_closed_form(oracle, pkg, dev, mode, bias, Nc, Nf):
    """Every weight zero and the sigma bias b: sigma = |b| at every sample.  The maps must be the fp64 evaluation of the definition over the
    call's own t_c / t_f (no oracle involved); 0 <= A <= 1 and near A <= D_c <= far A."""
    flags, B = MODES[mode]
    p = oracle.make_weights(0)
    for k in p:
        p[k] = torch.zeros_like(p[k])
    p["network.sigma_layer.0.bias"] = torch.full_like(p["network.sigma_layer.0.bias"], bias)
    P = [v.to(dev).contiguous() for v in p.values()]
    row, col, pb, K = _inputs(oracle, B, dev, seed=7)
    _, _, M, _, ws = _call(pkg, P, row, col, pb, K, Nc, Nf, flags, True)
    view = lambda name, n: pkg._abi.ws_view(ws, B, Nc, Nf, flags, name, (B, n)).double().cpu()
    t_c, t_f, sig_c = view("t_c", Nc), view("t_f", Nf), view("sig_c", Nc)
    assert torch.equal(sig_c, torch.full_like(sig_c, abs(bias)))
    near, far = pb[:, 15].double().cpu(), pb[:, 16].double().cpu()
    sigma = abs(bias)
    delta_c = ((far.float() - near.float()) / Nc).double()[:, None].expand(-1, Nc)  # quirk Q5, formed in fp32 as the kernel does
    w_c = _weights_fp64(delta_c, torch.full_like(t_c, sigma))
    t_s = torch.sort(torch.cat((t_c, t_f), 1), 1)[0]  # sigma is constant: the reference's channel sorts and the joint sort agree
    delta = torch.cat((t_s[:, 1:] - t_s[:, :-1], torch.full((B, 1), pkg.nerf.LAST_DELTA, dtype=torch.float64)), 1)
    w = _weights_fp64(delta, torch.full_like(t_s, sigma))
    ref = torch.stack(((w_c * t_c).sum(1), w_c.sum(1), (w * t_s).sum(1), w.sum(1)), 1)
    M = M.double().cpu()
    for j in range(4):
        assert max_rel(M[:, j], ref[:, j]) < 1e-5, (j, max_rel(M[:, j], ref[:, j]))
    A = M[:, 1::2]
    assert float(A.min()) >= 0.0 and float(A.max()) <= 1.0 + 1e-6
    Dc, Ac = M[:, 0], M[:, 1]
    assert bool((Dc >= near * Ac * (1 - 1e-6)).all()) and bool((Dc <= far * Ac * (1 + 1e-6)).all())


@pytest.mark.parametrize("mode", ["fp32", "bf16_pair"])
def test_render_maps_keep_the_batch_semantics(oracle, pkg, dev, mode):
    """render(maps=True) over a list whose batches have different near / far (fused calls, each handed its ray 0) and a one-ray tail: every
    ray's maps are the bits a per-batch maps call gives it, and the colours are render()'s."""
    Bm, Nc, Nf = 400, 64, 128
    n = 5 * Bm + 1
    row, col, pb, K, _ = oracle.fern_inputs(n, seed=12)
    p, _ = _weights_dev(oracle, 4, True, dev)
    m = pkg.NeRFModel(Nc, Nf, Bm)
    m.load_state_dict(p)
    m = m.to(dev)
    m.bf16_mlp = mode.startswith("bf16")
    rd, cd, pd = row.to(dev), col.to(dev), pb.float().to(dev)
    Cc0, Cf0 = m.render(rd, cd, pd, K)
    Cc, Cf, M = m.render(rd, cd, pd, K, maps=True)
    assert M.shape == (n, 4)
    assert torch.equal(Cc, Cc0) and torch.equal(Cf, Cf0)
    P = [v.detach() for v in m.network.parameters()]
    flags = pkg._abi.BF16_MLP if m.bf16_mlp else 0
    for s in range(0, n, Bm):
        e = min(s + Bm, n)
        r_, c_, p_ = rd[s:e], cd[s:e], pd[s:e]
        if e - s == 1:  # the library needs B >= 2: the ray twice, ray 0 = itself
            r_, c_, p_ = (torch.cat((x, x)) for x in (r_, c_, p_))
        c, f, Mb, _, _ = _call(pkg, P, r_.contiguous(), c_.contiguous(), p_.contiguous(), K, Nc, Nf, flags, True)
        assert torch.equal(M[s:e], Mb[: e - s]), s
        assert torch.equal(Cf[s:e], f[: e - s]), s


def _runner(pkg, tmp_path, bf16=False):
    scene = pkg.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    kw = dict(gpu=0, img_dir="", results_path=str(tmp_path) + "/res/", ckpt_path=str(tmp_path) + "/ck/", low_res=1, total_iter=1, batch_ray=256,
              learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1, decay_end=10000, sched="EXP",
              datasets={"train": scene, "val": scene, "test": scene}, log_every=1, bf16_mlp=bf16)
    torch.manual_seed(0)
    return pkg.NeRFRunner(continue_=False, **kw)


def test_display_writes_the_maps_and_keeps_the_frames(pkg, dev, tmp_path):
    run = _runner(pkg, tmp_path)
    frames = run.display(save=False)
    out = run.display(save=True, maps=True)
    assert isinstance(out, tuple) and len(out) == 3
    f2, depth, acc = out
    assert np.array_equal(frames, f2)
    pic, H, W = 3, 24, 24
    assert depth.shape == acc.shape == (pic, H, W) and depth.dtype == acc.dtype == np.float32
    # the pixels display() renders: the first (pic H W // batch) batches in pixel order; the tail stays white, NaN depth, 0 opacity
    n_keep = pic * H * W // 256 * 256
    rendered = np.zeros(pic * H * W, dtype=bool)
    rendered[:n_keep] = True
    rendered = rendered.reshape(pic, H, W)
    assert np.isfinite(depth[rendered]).all() and np.isnan(depth[~rendered]).all()
    assert (acc[~rendered] == 0).all() and (acc >= 0).all() and (acc <= 1 + 1e-6).all()
    z = np.load(glob.glob(str(tmp_path) + "/res/*_maps.npz")[0])
    assert np.array_equal(z["depth"], depth, equal_nan=True) and np.array_equal(z["acc"], acc)
    assert z["near"].shape == z["far"].shape == (pic,) and (z["near"] < z["far"]).all()
    for kind in ("depth", "acc"):
        assert len(glob.glob(str(tmp_path) + f"/res/*/*_{kind}.png")) == pic
    # the fine maps of display() are NeRFModel.render(maps=True)'s (the same calls the colours come from)
    rays = run.disp_rays
    row, col, _, poses_bound, pic_i = rays.gather(torch.arange(0, n_keep, device=run.device))
    m = run.model
    m.batch_ray = 256
    _, _, M = m.render(row, col, poses_bound, run.K_inv, maps=True)
    assert np.array_equal(depth[pic_i.cpu(), row.cpu(), col.cpu()], M[:, 2].cpu().numpy())
    assert np.array_equal(acc[pic_i.cpu(), row.cpu(), col.cpu()], M[:, 3].cpu().numpy())


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def _display_ranks(n, out, timeout=500):
    tool = os.path.join(ROOT, "tests", "tools", "maps_display_rank.py")
    env = _env()
    if n == 0:
        cmd = [sys.executable, tool, out]
    else:
        import socket

        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env["NERF_DIST_BACKEND"] = "gloo"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), tool, out]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "MAPS-DISPLAY-OK" in r.stdout
    return torch.load(os.path.join(out, "result.pt"), weights_only=False)


@pytest.mark.timeout(900)
def test_display_maps_tile_sharded_over_two_ranks_equal_one_rank(tmp_path):
    """display(maps=True) under a launcher, two ranks on the one GPU over gloo: the shards' maps travel through gather_rows (rows of width 4)
    and the assembled frames, depth and opacity are the single-process run's, bit for bit."""
    one = _display_ranks(0, str(tmp_path / "one"))
    two = _display_ranks(2, str(tmp_path / "two"))
    assert one["world"] == 1 and two["world"] == 2
    for k in ("frame", "depth", "acc"):
        assert torch.equal(one[k].nan_to_num(-1.0), two[k].nan_to_num(-1.0)), k
    assert torch.isnan(one["depth"]).any() and torch.isfinite(one["depth"]).any()
