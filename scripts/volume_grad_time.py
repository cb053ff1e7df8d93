"""Times fine-tuning a baked SH radiance volume on the analytic blob field of scripts/mesh_band_time.py baked
over [-3, 3]^3 at degree 2: per lattice size and batch, volume.render (forward), volume.render_backward into zeroed accumulators
(backward: rule VG, which marches twice and scatters) and ops.volume_adam_step (update: rule VU over the baked active list), each
between HIP events, medians after a warm-up.  Two batches per size: consecutive pixels of one image x image camera (neighbouring lanes
share cells) and pixels drawn at random from that camera's image (they do not).  Nothing is gated; the backward is read against the
forward of the same rays.  One JSON line per measurement.
Usage: python scripts/volume_grad_time.py [--sizes 128 256] [--rays 4096 65536] [--image 400] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402,F401
from nerf_tiny_amd import mesh, ops, volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def med(fn, reps):
    fn()
    return round(statistics.median(timed(fn) for _ in range(reps)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    blob = blob_model(dev)
    blob.eval()
    H = W = a.image
    pose = torch.zeros(1, 17)
    pose[0, :15] = torch.tensor([[1.0, 0, 0, 0.3, 0], [0, 1.0, 0, 0.2, 0], [0, 0, 1.0, 2.6, 0]]).reshape(-1)   # looks down -z from z = 2.6
    pose[0, 15:] = torch.tensor([0.5, 5.5])
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -1.1 * W]]).t().contiguous()
    o_all, d_all = mesh.camera_rays(pose, K_inv, H, W, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in a.sizes:
        vol = blob.bake_volume((-3.0,) * 3, (3.0,) * 3, n, degree=2, block=8)
        tuner = volume.Finetuner(vol)
        words = int(tuner.index.numel()) * 28
        print(json.dumps(dict(measure="memory", n=n, degree=2, active_points=int(tuner.index.numel()), lattice_points=n ** 3,
                              volume_MiB=round(n ** 3 * 112 / 2 ** 20, 1), accumulators_MiB=round(n ** 3 * 28 * 8 / 2 ** 20, 1),
                              moments_MiB=round(words * 8 / 2 ** 20, 1))), flush=True)
        for N in a.rays:
            for kind in ("one camera, consecutive pixels", "one camera, random pixels"):
                first = (H * W - N) // 2 if N <= H * W else 0
                idx = torch.arange(first, first + N, device=dev) % (H * W) if kind.endswith("consecutive pixels") else \
                    torch.randint(H * W, (N,), device=dev, generator=gen)
                o, d = o_all[idx].contiguous(), d_all[idx].contiguous()
                rgb, _, steps = volume.render(vol, o, d, 0.5, 5.5)
                g = (2.0 * (rgb - 0.5)).contiguous()
                grad = tuner.grad
                fwd = med(lambda: volume.render(vol, o, d, 0.5, 5.5), a.reps)

                def backward():
                    grad.acc_sigma.zero_(), grad.acc_coef.zero_()
                    volume.render_backward(vol, grad, o, d, 0.5, 5.5, g)

                zero = med(lambda: (grad.acc_sigma.zero_(), grad.acc_coef.zero_()), a.reps)
                bwd = med(backward, a.reps)
                step = [0]

                def update():
                    step[0] += 1
                    ops.volume_adam_step(tuner.vol.sigma, tuner.vol.coef, tuner.index, grad.acc_sigma, grad.acc_coef, tuner.m, tuner.v,
                                         1.0 / (3 * N), step[0], 0.0, 0.0)     # zero rates: the volume stays what the forward timed

                volume.render_backward(vol, grad, o, d, 0.5, 5.5, g)
                upd = med(update, a.reps)
                print(json.dumps(dict(measure="step", n=n, degree=2, rays=N, batch=kind, contributing=int(steps[:, 0].sum()),
                                      looked_at=int(steps[:, 1].sum()), forward_ms=fwd, zero_accumulators_ms=zero,
                                      backward_with_zeroing_ms=bwd, backward_ms=round(bwd - zero, 3),
                                      backward_over_forward=round((bwd - zero) / max(fwd, 1e-9), 2), update_ms=upd)), flush=True)
        del vol, tuner, grad


if __name__ == "__main__":
    main()
