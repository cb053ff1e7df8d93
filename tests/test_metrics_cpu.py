"""CPU: the fp64 restatement of the image metrics (tests/metrics_reference.py) and its closed forms, a cross-check of its filter against
scipy, the C ABI's refusals before any device work, the Python-side argument errors and the driver's --eval flags."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_reference as R  # noqa: E402


def test_window_is_normalised_gaussian():
    g = R.window()
    assert g.shape == (11,)
    assert abs(g.sum() - 1.0) < 1e-15
    np.testing.assert_allclose(g, g[::-1], rtol=0, atol=0)
    assert np.argmax(g) == 5
    np.testing.assert_allclose(g[4] / g[5], np.exp(-0.5 / 1.5 ** 2), rtol=1e-15)


@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.5, 0.5), (0.0, 1.0), (0.93, 0.05)])
def test_constant_images_closed_form(a, b):
    x = np.full((2, 17, 23, 3), a)
    y = np.full((2, 17, 23, 3), b)
    mse, ssim = R.metrics(x, y)
    np.testing.assert_allclose(mse, (a - b) ** 2, rtol=1e-15, atol=0)
    np.testing.assert_allclose(ssim, (2 * a * b + R.C1) / (a * a + b * b + R.C1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("d", [0.1, -0.03, 0.25])
def test_constant_offset_psnr(d):
    from nerf_tiny_amd.metrics import psnr_from_mse

    rng = np.random.default_rng(1)
    x = rng.uniform(0.3, 0.6, (1, 12, 14, 3))
    mse, _ = R.metrics(x + d, x)
    np.testing.assert_allclose(psnr_from_mse(mse), -20 * np.log10(abs(d)), rtol=1e-12)


def test_identical_images():
    rng = np.random.default_rng(2)
    x = rng.uniform(0, 1, (3, 20, 30, 3))
    mse, ssim = R.metrics(x, x)
    assert (mse == 0).all()
    np.testing.assert_allclose(ssim, 1.0, rtol=0, atol=1e-15)


def test_psnr_from_mse():
    from nerf_tiny_amd.metrics import psnr_from_mse

    assert psnr_from_mse(0.0) == float("inf")
    assert psnr_from_mse(1e-2) == pytest.approx(20.0, rel=1e-15)
    assert np.isnan(psnr_from_mse(float("nan")))
    out = psnr_from_mse(np.array([1.0, 1e-3, 0.0]))
    np.testing.assert_allclose(out, [0.0, 30.0, np.inf], rtol=1e-15)


def test_nan_reaches_ssim_and_mse():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (2, 15, 15, 3))
    y = x.copy()
    y[1, 0, 14, 2] = np.nan  # a corner pixel: inside exactly one valid window
    mse, ssim = R.metrics(x, y)
    assert np.isfinite(mse[0]) and np.isfinite(ssim[0])
    assert np.isnan(mse[1]) and np.isnan(ssim[1])


def test_filter_matches_scipy_convolve2d():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(4)
    z = rng.uniform(0, 1, (1, 31, 44, 3))
    g = R.window()
    ours = R.filt(z)
    for c in range(3):
        ref = signal.convolve2d(signal.convolve2d(z[0, :, :, c], g[None, :], mode="valid"), g[:, None], mode="valid")
        np.testing.assert_allclose(ours[0, :, :, c], ref, rtol=0, atol=1e-14)
    assert ours.shape == (1, 21, 34, 3)


# ----- the C ABI: refusals before any device work (pointer values only: nothing is dereferenced) -----
def _metrics(pkg, n, H, W, pred=1, gt=1, mse=1, ssim=1, ws=1 << 20, ws_bytes=1 << 40):
    p = lambda v: ctypes.c_void_p(v << 12) if v else None
    return pkg._abi.lib().nerf_hip_image_metrics(p(pred), p(gt), n, H, W, p(mse), p(ssim), ctypes.c_void_p(ws) if ws else None, ws_bytes,
                                                  None)


def test_metrics_abi_declared_and_ws_bytes(pkg):
    assert "nerf_hip_image_metrics" in pkg._abi.EXPORTS and "nerf_hip_metrics_ws_bytes" in pkg._abi.EXPORTS
    lib = ctypes.CDLL(pkg._abi.LIB_PATH)
    assert hasattr(lib, "nerf_hip_image_metrics") and hasattr(lib, "nerf_hip_metrics_ws_bytes")
    assert pkg._abi.lib().nerf_hip_abi_version() == 7
    # 16 bytes per (view, tile of 16 x 32 valid outputs), rounded to 256
    assert pkg._abi.metrics_ws_bytes(1, 11, 11) == 256
    assert pkg._abi.metrics_ws_bytes(3, 800, 800) == -(-3 * 50 * 25 * 16 // 256) * 256
    assert pkg._abi.metrics_ws_bytes(0, 64, 64) == 0
    for n, H, W in ((-1, 64, 64), (1, 10, 64), (1, 64, 10), (1, 30000, 30000)):
        with pytest.raises(pkg._abi.NerfHipError):
            pkg._abi.metrics_ws_bytes(n, H, W)


@pytest.mark.parametrize("kw,match", [
    (dict(n=-1), "n=-1"),
    (dict(H=10), "window"),
    (dict(W=3), "window"),
    (dict(H=30000, W=30000), "2\\^31"),
    (dict(pred=0), "null"),
    (dict(gt=0), "null"),
    (dict(mse=0), "null"),
    (dict(ssim=0), "null"),
    (dict(ws=0), "workspace is null"),
    (dict(ws=(1 << 20) + 8), "aligned"),
    (dict(ws_bytes=255), "workspace"),
])
def test_metrics_refusals(pkg, kw, match):
    args = dict(n=2, H=64, W=64)
    args.update(kw)
    rc = _metrics(pkg, **args)
    assert rc != 0
    with pytest.raises(pkg._abi.NerfHipError, match=match):
        pkg._abi.check(rc)


def test_metrics_n_zero_is_a_noop(pkg):
    assert _metrics(pkg, 0, 64, 64, pred=0, gt=0, mse=0, ssim=0, ws=0, ws_bytes=0) == 0


# ----- Python-side argument errors (raised before anything reaches a device) -----
def test_image_metrics_argument_errors(pkg):
    M = pkg.metrics
    a = np.zeros((2, 16, 16, 3), np.float32)
    with pytest.raises(ValueError, match="differ"):
        M.image_metrics(a, a[:1])
    with pytest.raises(ValueError, match="\\[H, W, 3\\]"):
        M.image_metrics(a[..., :2], a[..., :2])
    with pytest.raises(ValueError, match="window"):
        M.image_metrics(a[:, :10], a[:, :10])
    with pytest.raises(TypeError):
        M.image_metrics([[0.0]], [[0.0]])
    import torch

    t = torch.zeros(2, 16, 16, 3)
    with pytest.raises(ValueError, match="same shape"):
        pkg.ops.image_metrics(t, t[:, :15])
    with pytest.raises(ValueError, match="same shape"):
        pkg.ops.image_metrics(t[0], t[0])
    with pytest.raises(ValueError, match="ROCm device"):
        pkg.ops.image_metrics(t, t)  # host tensors never reach the kernels


def test_runner_argument_errors(pkg):
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="eval_every"):
            pkg.NeRFRunner(eval_every=bad)
    for bad in ([], [1.0], "x"):
        with pytest.raises(ValueError, match="views"):
            pkg.NeRFRunner(eval_every=10, eval_views=bad)


def test_cli_eval_flags():
    src = open(os.path.join(ROOT, "nerf-tiny_amd", "main.py")).read()
    assert 'run.evaluate("disp", views=args.eval_views, save=True)' in src
    ap = importlib.import_module("nerf_tiny_amd.main").build_parser()
    a = ap.parse_args([])
    assert a.eval is False and a.eval_every is None and a.eval_views is None
    a = ap.parse_args(["--eval", "--eval-every", "100", "--eval-views", "0", "3", "7"])
    assert a.eval is True and a.eval_every == 100 and a.eval_views == [0, 3, 7]
    with pytest.raises(SystemExit):
        ap.parse_args(["--eval-every", "x"])
    with pytest.raises(SystemExit):
        ap.parse_args(["--eval-views"])
