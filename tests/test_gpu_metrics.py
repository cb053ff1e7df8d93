"""GPU: nerf_hip_image_metrics (per-view MSE and SSIM in fp64, csrc/metrics.hip) against the numpy restatement (tests/metrics_reference.py),
its edge cases, determinism and refusals; NeRFRunner.evaluate (frames, metrics, JSON, views), the training-loop hook (eval_every leaves
training bit-identical) and a two-rank evaluation over gloo."""
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _images(n, H, W, kind, seed):
    """(pred, gt) float32 [n, H, W, 3]: random, or structured (gradients, a checkerboard, flat patches, saturated 0 / 1, a noisy copy)."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(0, 1, (n, H, W, 3)).astype(np.float32), rng.uniform(0, 1, (n, H, W, 3)).astype(np.float32)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    gt = np.empty((n, H, W, 3))
    for v in range(n):
        gt[v, ..., 0] = (xx + 0.3 * v) % 1.0
        gt[v, ..., 1] = ((np.arange(H)[:, None] // 4 + np.arange(W)[None, :] // 4 + v) % 2).astype(np.float64)
        gt[v, ..., 2] = 0.5
    gt[:, : H // 3, : W // 3] = 1.0  # a flat white patch: the cancellation E[x^2] - E[x]^2 in fp64
    pred = np.clip(gt + 0.02 * rng.standard_normal(gt.shape), 0, 1)
    pred[:, H // 2:, W // 2:, 2] = 0.0
    return pred.astype(np.float32), gt.astype(np.float32)


@pytest.mark.parametrize("n,H,W", [(1, 11, 11), (3, 12, 37), (2, 64, 64), (7, 33, 129), (1, 800, 800)])
@pytest.mark.parametrize("kind", ["random", "structured"])
def test_metrics_match_the_fp64_restatement(pkg, dev, n, H, W, kind):
    pred, gt = _images(n, H, W, kind, seed=n * 1000 + H)
    mse, ssim = pkg.ops.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
    assert mse.dtype == ssim.dtype == torch.float64 and mse.shape == ssim.shape == (n,)
    rmse, rssim = R.metrics(pred, gt)
    np.testing.assert_allclose(mse.cpu().numpy(), rmse, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ssim.cpu().numpy(), rssim, rtol=0, atol=1e-12)
    # the metrics module: the same numbers per view, PSNR from them; [H, W, 3] input gives floats
    d = pkg.metrics.image_metrics(pred, gt)
    assert np.array_equal(d["mse"], mse.cpu().numpy()) and np.array_equal(d["ssim"], ssim.cpu().numpy())
    assert np.array_equal(d["psnr"], -10 * np.log10(d["mse"]))
    one = pkg.metrics.image_metrics(torch.from_numpy(pred[-1]).to(dev), gt[-1])
    assert one["mse"] == d["mse"][-1] and one["ssim"] == d["ssim"][-1] and isinstance(one["psnr"], float)


def test_identical_images_and_constant_closed_form(pkg, dev):
    x = torch.rand(3, 40, 52, 3, device=dev)
    mse, ssim = pkg.ops.image_metrics(x, x.clone())
    assert (mse == 0).all()
    assert float((ssim - 1).abs().max()) <= 1e-15
    assert pkg.metrics.image_metrics(x, x)["psnr"].tolist() == [float("inf")] * 3
    for a, b in ((0.2, 0.7), (0.0, 1.0), (0.93, 0.05), (0.5, 0.5)):
        p = torch.full((2, 23, 17, 3), a, device=dev)
        g = torch.full((2, 23, 17, 3), b, device=dev)
        mse, ssim = pkg.ops.image_metrics(p, g)
        fa, fb = float(np.float32(a)), float(np.float32(b))  # the fp32 values the kernel reads
        np.testing.assert_allclose(mse.cpu().numpy(), (fa - fb) ** 2, rtol=1e-15)
        np.testing.assert_allclose(ssim.cpu().numpy(), (2 * fa * fb + R.C1) / (fa * fa + fb * fb + R.C1), rtol=0, atol=1e-12)


def test_nan_and_inf_stay_in_their_view(pkg, dev):
    pred, gt = _images(4, 30, 41, "random", seed=7)
    clean = [t.cpu().numpy() for t in pkg.ops.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))]
    pred[1, 0, 40, 2] = np.nan  # a corner pixel: inside one valid window only
    gt[2, 15, 20, 0] = np.inf
    mse, ssim = (t.cpu().numpy() for t in pkg.ops.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)))
    for v in (0, 3):
        assert mse[v] == clean[0][v] and ssim[v] == clean[1][v]
    assert np.isnan(mse[1]) and np.isnan(ssim[1])
    assert np.isinf(mse[2]) and np.isnan(ssim[2])


def test_deterministic_and_independent_of_the_workspace(pkg, dev):
    pred, gt = (torch.from_numpy(a).to(dev) for a in _images(3, 200, 300, "structured", seed=3))
    nbytes = pkg._abi.metrics_ws_bytes(3, 200, 300)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    a = pkg.ops.image_metrics(pred, gt, ws=ws)
    ws.view(torch.float64).fill_(float("nan"))
    b = pkg.ops.image_metrics(pred, gt, ws=ws)
    ws.random_(0, 256)
    c = pkg.ops.image_metrics(pred, gt, ws=ws)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    # a view's result does not depend on the other views of the call
    m1, s1 = pkg.ops.image_metrics(pred[1:2], gt[1:2])
    assert torch.equal(m1, a[0][1:2]) and torch.equal(s1, a[1][1:2])


def test_refusals_leave_the_outputs_alone(pkg, dev):
    L = pkg._abi.lib()
    n, H, W = 2, 32, 32
    pred = torch.rand(n, H, W, 3, device=dev)
    gt = torch.rand(n, H, W, 3, device=dev)
    mse = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    ssim = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    need = pkg._abi.metrics_ws_bytes(n, H, W)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: t.data_ptr()
    cases = [
        (P(pred), P(gt), -1, H, W, P(mse), P(ssim), P(ws), need),
        (P(pred), P(gt), n, 10, W, P(mse), P(ssim), P(ws), need),
        (P(pred), P(gt), n, H, 10, P(mse), P(ssim), P(ws), need),
        (P(pred), P(gt), n, 40000, 40000, P(mse), P(ssim), P(ws), ws.numel()),
        (None, P(gt), n, H, W, P(mse), P(ssim), P(ws), need),
        (P(pred), None, n, H, W, P(mse), P(ssim), P(ws), need),
        (P(pred), P(gt), n, H, W, None, P(ssim), P(ws), need),
        (P(pred), P(gt), n, H, W, P(mse), None, P(ws), need),
        (P(pred), P(gt), n, H, W, P(mse), P(ssim), None, need),
        (P(pred), P(gt), n, H, W, P(mse), P(ssim), P(ws) + 8, need),
        (P(pred), P(gt), n, H, W, P(mse), P(ssim), P(ws), need - 1),
    ]
    for args in cases:
        assert L.nerf_hip_image_metrics(*args, st) != 0, args
    assert L.nerf_hip_image_metrics(None, None, 0, H, W, None, None, None, 0, st) == 0  # n == 0: a no-op
    torch.cuda.synchronize()
    assert (mse == -7.0).all() and (ssim == -7.0).all()
    assert L.nerf_hip_image_metrics(P(pred), P(gt), n, H, W, P(mse), P(ssim), P(ws), need, st) == 0  # the exact size is enough
    torch.cuda.synchronize()
    assert (mse != -7.0).all() and (ssim != -7.0).all()
    e, s = pkg.ops.image_metrics(pred[:0], gt[:0])
    assert e.shape == s.shape == (0,)


# ----- the runner -----
def _runner(pkg, tmp_path, name="a", **extra):
    scene = pkg.data.analytic_sphere_scene(n_pic=4, H=32, W=32, seed=5, device="cuda:0")
    kw = dict(gpu=0, img_dir="", results_path=str(tmp_path) + f"/{name}/res/", ckpt_path=str(tmp_path) + f"/{name}/ck/", low_res=1, total_iter=1,
              batch_ray=300, learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=10 ** 9,
              decay_end=10000, sched="EXP", datasets={"train": scene, "val": scene, "test": scene}, log_every=10 ** 9, on_resample_fault="warn")
    kw.update(extra)
    torch.manual_seed(0)
    return pkg.NeRFRunner(continue_=False, **kw), scene


def test_evaluate_renders_displays_pixels_and_scores_them(pkg, dev, tmp_path):
    run, scene = _runner(pkg, tmp_path)
    frames = run.display(save=False)
    pic, H, W = 4, 32, 32
    n_keep = pic * H * W // 300 * 300  # display() leaves the last 196 pixels white; evaluate renders them
    shown = np.zeros(pic * H * W, dtype=bool)
    shown[:n_keep] = True
    shown = shown.reshape(pic, H, W)
    gts = scene.all_pix.view(pic, H, W, 3)
    views = []
    for i in range(pic):
        frame, gt = run.render_view(i)
        assert frame.shape == gt.shape == (H, W, 3)
        assert np.array_equal(frame.cpu().numpy()[shown[i]], frames[i][shown[i]]), i
        assert torch.equal(gt.cpu(), gts[i])
        views.append((frame, gt))
    assert not np.array_equal(frames[-1][~shown[-1]], views[-1][0].cpu().numpy()[~shown[-1]])  # the tail is rendered, not white
    r = run.evaluate(save=True)
    assert r["mode"] == "disp" and r["views"] == [0, 1, 2, 3] and r["iter"] == run.last_iter and r["seconds"] > 0
    for i, (frame, gt) in enumerate(views):
        mse, ssim = pkg.ops.image_metrics(frame[None], gt[None])
        pv = r["per_view"][i]
        assert pv["view"] == i and pv["mse"] == float(mse) and pv["ssim"] == float(ssim)
        assert pv["psnr"] == float(-10 * np.log10(float(mse)))
    assert r["psnr"] == float(np.mean([v["psnr"] for v in r["per_view"]]))
    assert r["ssim"] == float(np.mean([v["ssim"] for v in r["per_view"]]))
    assert r["mse"] == float(np.mean([v["mse"] for v in r["per_view"]]))
    files = glob.glob(str(tmp_path) + "/a/res/*_eval.json")
    assert len(files) == 1 and files[0].endswith(f"_{run.last_iter}_eval.json")
    assert json.load(open(files[0])) == json.loads(json.dumps(r))
    r2 = run.evaluate(views=[2, 0], save=False)
    assert r2["views"] == [2, 0] and [v["view"] for v in r2["per_view"]] == [2, 0]
    assert r2["per_view"][0] == {**r["per_view"][2]} and r2["per_view"][1] == r["per_view"][0]
    assert len(glob.glob(str(tmp_path) + "/a/res/*_eval.json")) == 1
    for bad in ("test", "bogus"):
        with pytest.raises(ValueError, match="mode"):
            run.evaluate(bad)
    with pytest.raises(ValueError, match="views"):
        run.evaluate(views=[4])


def test_evaluate_leaves_no_bit_in_the_sticky_status(pkg, dev, tmp_path):
    """Rays of an evaluation that meet the resample condition (sigma = 0 everywhere: every ray's coarse weights vanish) leave nothing
    for resample_fault_since to find; display()'s rays on the model's own workspaces do."""
    run, _ = _runner(pkg, tmp_path)
    with torch.no_grad():
        run.model.network.sigma_layer[0].weight.zero_()
        run.model.network.sigma_layer[0].bias.zero_()
    assert run.model.training
    run.evaluate(views=[1], save=False)
    assert run.model.training  # the train / eval mode is pickled into checkpoints: it comes back
    assert not run.model.resample_fault_since(clear=False)
    run.display(save=False)
    assert run.model.resample_fault_since(clear=True)


class _Recorder:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, it):
        self.scalars.append((tag, value, it))

    def flush(self):
        pass


def test_eval_every_leaves_training_bit_identical(pkg, dev, tmp_path, capsys):
    kw = dict(total_iter=40, step=20, log_every=10, batch_ray=256, learning=3e-3)
    a, _ = _runner(pkg, tmp_path, "a", **kw)
    b, _ = _runner(pkg, tmp_path, "b", eval_every=10, eval_views=[0, 3], **kw)
    for x, y in zip(a.model.network.parameters(), b.model.network.parameters()):
        assert torch.equal(x, y)
    a.writer, b.writer = _Recorder(), _Recorder()
    assert a.trainer("train") == b.trainer("train") == 39
    out = capsys.readouterr().out
    assert out.count("[EVAL]") == 4
    for x, y in zip(a.model.network.parameters(), b.model.network.parameters()):
        assert torch.equal(x, y)
    assert torch.equal(a.optimizer._m, b.optimizer._m) and torch.equal(a.optimizer._v, b.optimizer._v)
    assert a.optimizer._step == b.optimizer._step == 40
    assert torch.equal(a.train_rays.gen.get_state(), b.train_rays.gen.get_state())
    assert a.resample_fault_iter == b.resample_fault_iter
    assert a.model.training and b.model.training and b.model.batch_ray == a.model.batch_ray
    evals = [s for s in b.writer.scalars if s[0] in ("psnr/val", "ssim/val")]
    assert [(t, it) for t, _, it in evals] == [(t, it) for it in (9, 19, 29, 39) for t in ("psnr/val", "ssim/val")]
    assert all(np.isfinite(v) for _, v, _ in evals)
    assert [s for s in b.writer.scalars if s[0] not in ("psnr/val", "ssim/val")] == a.writer.scalars  # losses and learning rates
    for it in (19, 39):
        (fa,), (fb,) = (glob.glob(str(tmp_path) + f"/{n}/ck/*_{it}.pkl") for n in ("a", "b"))
        ma, mb = torch.load(fa, weights_only=False, map_location=dev), torch.load(fb, weights_only=False, map_location=dev)
        assert ma.training == mb.training and ma.batch_ray == mb.batch_ray
        for (k, x), y in zip(ma.state_dict().items(), mb.state_dict().values()):
            assert torch.equal(x, y), k
        oa, ob = (torch.load(f[:-4] + ".opt", weights_only=False) for f in (fa, fb))
        assert oa["sampler"]["next_batch"] == ob["sampler"]["next_batch"]
        assert torch.equal(oa["sampler"]["epoch_gen_state"], ob["sampler"]["epoch_gen_state"])
        assert oa["adam"]["step"] == ob["adam"]["step"]
        assert torch.equal(oa["adam"]["exp_avg"], ob["adam"]["exp_avg"]) and torch.equal(oa["adam"]["exp_avg_sq"], ob["adam"]["exp_avg_sq"])


def _eval_ranks(n, out, timeout=500):
    tool = os.path.join(ROOT, "tests", "tools", "eval_rank.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    if n == 0:
        cmd = [sys.executable, tool, out]
    else:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        env["NERF_DIST_BACKEND"] = "gloo"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), tool, out]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("EVAL-RANK-OK") == max(n, 1)
    return [torch.load(f, weights_only=False) for f in sorted(glob.glob(os.path.join(out, "rank*.pt")))]


@pytest.mark.timeout(900)
def test_evaluate_over_two_ranks_equals_one_rank(tmp_path):
    """evaluate() under a launcher, two ranks on the one GPU over gloo: the views' reference batches are dealt out as display() deals them,
    rank 0 scores the gathered frames, and the metrics are the single-process run's, bit for bit; rank 1 returns None."""
    (one,) = _eval_ranks(0, str(tmp_path / "one"))
    two, two_r1 = _eval_ranks(2, str(tmp_path / "two"))
    assert one["world"] == 1 and two["world"] == two_r1["world"] == 2 and two_r1["result"] is None
    assert one["result"]["per_view"] == two["result"]["per_view"]
    for k in ("psnr", "ssim", "mse", "views", "iter", "mode"):
        assert one["result"][k] == two["result"][k], k
    assert torch.equal(one["frame"], two["frame"]) and torch.equal(one["frame"], two_r1["frame"])
