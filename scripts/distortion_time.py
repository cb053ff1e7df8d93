"""Times one training step with and without the distortion loss: forward(maps=True) + ray_loss + backward() against
forward(maps=True, distortion=True) + ray_loss + 0.01 * distortion_loss + backward(), at 4096 and 400 rays (64 + 128 samples), in exact fp32
and with the bf16 MLP.  Both steps alternate in one process on one build, HIP events around each, after a warm-up of both; the maps step's
kernels are untouched by the feature, so the difference is the maps + distortion forms of k_coarse_x / k_merge_x and of k_merge_bwd_x /
k_coarse_bwd_x against their maps forms, and the [B, 2] output and its sum.  Prints one JSON line per case (median ms
of each step and the ratio).
Usage: python scripts/distortion_time.py [--reps 30]"""
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

LAMBDA = 0.01


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (4096, 400):
        row, col, pb, K, Ct = O.lego_inputs(B)
        row, col, pb, Ct = row.to(dev), col.to(dev), pb.float().to(dev), Ct.float().to(dev)
        m = P.NeRFModel(64, 128, B)
        m.load_state_dict(O.make_weights(4, sharp=True))
        m = m.to(dev)
        for kind in ("fp32", "bf16"):
            m.bf16_mlp = kind == "bf16"

            def maps_step():
                m.zero_grad(set_to_none=True)
                Cc, Cf, _ = m(row, col, pb, K, maps=True)
                m.ray_loss(Cc, Cf, Ct).backward()

            def dist_step():
                m.zero_grad(set_to_none=True)
                Cc, Cf, _, D = m(row, col, pb, K, maps=True, distortion=True)
                (m.ray_loss(Cc, Cf, Ct) + LAMBDA * m.distortion_loss(D)).backward()

            for _ in range(3):
                timed(maps_step), timed(dist_step)
            t0, t1 = [], []
            for _ in range(a.reps):
                t0.append(timed(maps_step))
                t1.append(timed(dist_step))
            m0, m1 = statistics.median(t0), statistics.median(t1)
            print(json.dumps(dict(case=f"{kind}_{B}", rays=B, maps_step_ms=round(m0, 3), distortion_step_ms=round(m1, 3), ratio=round(m1 / m0, 4),
                                  maps_min_ms=round(min(t0), 3), distortion_min_ms=round(min(t1), 3), reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
