"""Times NeRFModel.render(maps=True) on one 400 x 400 frame (batch_ray 400) with and without quantiles=(0.25, 0.5, 0.75) (DESIGN.md section
3i-2), for the exact fp32, split-fp32 and bf16-MLP inference kernels: the two versions alternate in one process, HIP events around each
render, after a warm-up of both.  Two call layouts per precision, as scripts/maps_time.py: the frame's batches fused into 16,384-ray calls
(render's default) and one call per 400-ray batch (fuse_rays=400).  Both versions take the separate k_coarse / k_merge launches, so the
difference is the quantile loop of the maps + quantiles forms of k_coarse_x / k_merge_x and the [n, 2, 3] output.  Prints one JSON line per case (median ms of
each version and the ratio).
Usage: python scripts/quantile_time.py [--reps 10]"""
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

QUANTILES = (0.25, 0.5, 0.75)


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
    row, col, pb, K, _ = O.lego_inputs(H * W, H=H, W=W, crop=H)  # every pixel of the frame
    row, col, pb = row.to(dev), col.to(dev), pb.float().to(dev)
    m = P.NeRFModel(64, 128, 400)
    m.load_state_dict(O.make_weights(4, sharp=True))
    m = m.to(dev)
    for kind in ("fp32", "split", "bf16"):
        m.split_mlp, m.bf16_mlp = kind == "split", kind == "bf16"
        for fuse in (16384, 400):
            maps = lambda: m.render(row, col, pb, K, fuse_rays=fuse, maps=True)
            quant = lambda: m.render(row, col, pb, K, fuse_rays=fuse, maps=True, quantiles=QUANTILES)
            for _ in range(2):
                timed(maps), timed(quant)
            t0, t1 = [], []
            for _ in range(a.reps):
                t0.append(timed(maps))
                t1.append(timed(quant))
            m0, m1 = statistics.median(t0), statistics.median(t1)
            print(json.dumps(dict(case=f"{kind}_fuse{fuse}", rays=H * W, maps_ms=round(m0, 3), quantiles_ms=round(m1, 3), ratio=round(m1 / m0, 4),
                                  maps_min_ms=round(min(t0), 3), quantiles_min_ms=round(min(t1), 3))), flush=True)


if __name__ == "__main__":
    main()
