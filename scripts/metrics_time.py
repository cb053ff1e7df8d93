"""Times nerf_hip_image_metrics (MSE + SSIM, fp64) on 800 x 800 views against the fp32 render of one such view
(NeRFModel.render, batch_ray 400, every pixel of the frame): HIP events around each call after a warm-up; prints one JSON line with the
median ms per view of both and their ratio.  Kernel times come from a separate profiler run: --metrics-only skips the render.
Usage: python scripts/metrics_time.py [--reps 50] [--views 1] [--metrics-only]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nerf_oracle as O  # noqa: E402

import nerf_tiny_amd as P  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--metrics-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 800
    gen = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(a.views, H, W, 3, device=dev, generator=gen)
    pred = (gt + 0.05 * torch.randn(a.views, H, W, 3, device=dev, generator=gen)).clamp(0, 1)
    ws = torch.empty(P._abi.metrics_ws_bytes(a.views, H, W), dtype=torch.uint8, device=dev)
    call = lambda: P.ops.image_metrics(pred, gt, ws=ws)
    for _ in range(5):
        timed(call)
    tm = statistics.median(timed(call) for _ in range(a.reps))
    out = dict(case=f"image_metrics {a.views} x {H}x{W}", metrics_ms_per_view=round(tm / a.views, 4))
    if not a.metrics_only:
        row, col, pb, K, _ = O.lego_inputs(H * W, H=H, W=W, crop=H)  # every pixel of one frame
        row, col, pb = row.to(dev), col.to(dev), pb.float().to(dev)
        m = P.NeRFModel(64, 128, 400)
        m.load_state_dict(O.make_weights(4, sharp=True))
        m = m.to(dev)
        render = lambda: m.render(row, col, pb, K)
        timed(render)
        tr = statistics.median(timed(render) for _ in range(3))
        out.update(render_fp32_ms_per_view=round(tr, 1), ratio=round(tm / a.views / tr, 6))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
