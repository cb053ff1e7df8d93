"""Times the point-gradient query: query_grad(points) (sigma only, the gradient of sigma) and the colour VJP
query_grad(points, dirs, dsigma, drgb), beside query() alone at the same points in the same process for the ratio.  HIP events after
warm-up, pack and both launches included.  Prints one JSON line per case.  Usage: python scripts/query_grad_time.py [--reps 10] [--M 1048576]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402

PEAK = 157.3e12  # fp32 MFMA, FLOP/s
FLOP_MFMA = 32 * 32 * 2 * 2  # v_mfma_f32_32x32x2f32


def events_ms(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--M", type=int, default=1 << 20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    M = a.M
    pts = torch.rand(M, 3, device=dev) * 8.0 - 4.0
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device=dev), dim=1)
    u, v = torch.randn(M, device=dev), torch.randn(M, 3, device=dev)
    # MFMAs per 32 points executed by each kernel (field_fwd_reg.hip / field_bwd_reg.hip)
    cases = [
        ("query", lambda: model.query(pts), 7744),
        ("query_grad", lambda: model.query_grad(pts), 7744 + 7688),
        ("query_rgb", lambda: model.query(pts, dirs), 8256),
        ("query_grad_vjp_rgb", lambda: model.query_grad(pts, dirs, dsigma=u, drgb=v), 8256 + 8200),
    ]
    base = {}
    for name, fn, mfma in cases:
        t = events_ms(fn, a.reps)
        out = dict(case=name, M=M, ms=round(t, 3), Mpts_per_s=round(M / t / 1e3, 1),
                   peak_share=round(M / 32 * mfma * FLOP_MFMA / (t * 1e-3) / PEAK, 3))
        if name.startswith("query_grad"):
            out["ratio_to_query"] = round(t / base["query_rgb" if "rgb" in name else "query"], 3)
        base[name] = t
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
