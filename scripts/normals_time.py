"""Times NeRFModel.render(maps=True) on one 400 x 400 frame (batch_ray 400) with and without normals="fine" / "both" (DESIGN.md section
3i-3), for the exact fp32, split-fp32 and bf16-MLP inference kernels: the three versions alternate in one process, HIP events around each
render, after a warm-up of all.  The frame's batches are fused into 16,384-ray calls (render's default).  All versions take the separate
k_coarse / k_merge launches, so the difference is the gradient query over the call's own sample points (exact fp32 in every row), the
points / normal-composite kernels around it and the [n, 2, 3] output.  Prints one JSON line per precision (median ms of each version, the
ratios to the maps frame, the gradient points per second the additions come to) and one with the side workspace's size at 16,384 rays.
Usage: python scripts/normals_time.py [--reps 10]"""
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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 400
    Nc, Nf = 64, 128
    row, col, pb, K, _ = O.lego_inputs(H * W, H=H, W=W, crop=H)  # every pixel of the frame
    row, col, pb = row.to(dev), col.to(dev), pb.float().to(dev)
    m = P.NeRFModel(Nc, Nf, 400)
    m.load_state_dict(O.make_weights(4, sharp=True))
    m = m.to(dev)
    print(json.dumps(dict(side_workspace_bytes_16384_rays=P._abi.normals_ws_bytes(16384, Nc, Nf),
                          main_workspace_bytes_16384_rays=P._abi.ws_bytes(16384, Nc, Nf, 0))), flush=True)
    for kind in ("fp32", "split", "bf16"):
        m.split_mlp, m.bf16_mlp = kind == "split", kind == "bf16"
        runs = {"maps": lambda: m.render(row, col, pb, K, maps=True),
                "fine": lambda: m.render(row, col, pb, K, maps=True, normals="fine"),
                "both": lambda: m.render(row, col, pb, K, maps=True, normals="both")}
        for _ in range(2):
            for fn in runs.values():
                timed(fn)
        t = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                t[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in t.items()}
        pts = {"fine": H * W * (Nc + Nf), "both": H * W * (2 * Nc + Nf)}
        print(json.dumps(dict(case=kind, rays=H * W, maps_ms=round(med["maps"], 3), fine_ms=round(med["fine"], 3), both_ms=round(med["both"], 3),
                              fine_ratio=round(med["fine"] / med["maps"], 3), both_ratio=round(med["both"] / med["maps"], 3),
                              fine_Mpts_per_s=round(pts["fine"] / (med["fine"] - med["maps"]) / 1e3, 1),
                              both_Mpts_per_s=round(pts["both"] / (med["both"] - med["maps"]) / 1e3, 1),
                              maps_min_ms=round(min(t["maps"]), 3), fine_min_ms=round(min(t["fine"]), 3), both_min_ms=round(min(t["both"]), 3))),
              flush=True)


if __name__ == "__main__":
    main()
