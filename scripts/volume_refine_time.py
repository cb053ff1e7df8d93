"""Times the coarse-to-fine pieces of volume fine-tuning on the analytic blob field of
scripts/mesh_band_time.py baked over [-3, 3]^3 at degree 2: per lattice size volume.tv_backward (rule VT over the active list) beside
ops.volume_adam_step (rule VU over the same list) and volume.render_backward of 65,536 rays of the same run, then volume.member_mask,
volume.prune (rule VP, with its copies and without) and volume.upsample (rule VX) of the smaller sizes.  HIP events, medians after a
warm-up.  Nothing is gated.  One JSON line per measurement.
Usage: python scripts/volume_refine_time.py [--sizes 128 256] [--upsample 128] [--rays 65536] [--image 400] [--reps 7]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402,F401
from nerf_tiny_amd import mesh, ops, volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402
from volume_grad_time import med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--upsample", type=int, nargs="+", default=[128])
    ap.add_argument("--rays", type=int, default=65536)
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
    N = a.rays
    idx = torch.randint(H * W, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    o, d = o_all[idx].contiguous(), d_all[idx].contiguous()
    for n in a.sizes:
        vol = blob.bake_volume((-3.0,) * 3, (3.0,) * 3, n, degree=2, block=8)
        tuner = volume.Finetuner(vol, tv_sigma=1e-3, tv_coef=1e-3)
        grad, members = tuner.grad, int(tuner.index.numel())
        g = (2.0 * (volume.render(vol, o, d, 0.5, 5.5)[0] - 0.5)).contiguous()
        zero = med(lambda: (grad.acc_sigma.zero_(), grad.acc_coef.zero_()), a.reps)

        def backward():
            grad.acc_sigma.zero_(), grad.acc_coef.zero_()
            volume.render_backward(vol, grad, o, d, 0.5, 5.5, g)

        bwd = med(backward, a.reps)
        k = 3.0 * N / max(members, 1)
        tv = med(lambda: volume.tv_backward(tuner.vol, grad, tuner.index, tuner.member, 1e-3 * k, 1e-3 * k), a.reps)
        tv_sigma_only = med(lambda: volume.tv_backward(tuner.vol, grad, tuner.index, tuner.member, 1e-3 * k, 0.0), a.reps)
        step = [0]

        def update():
            step[0] += 1
            ops.volume_adam_step(tuner.vol.sigma, tuner.vol.coef, tuner.index, grad.acc_sigma, grad.acc_coef, tuner.m, tuner.v,
                                 1.0 / (3 * N), step[0], 0.0, 0.0)     # zero rates: the volume stays what was timed

        upd = med(update, a.reps)
        mask = med(lambda: volume.member_mask(tuner.vol, tuner.index), a.reps)
        print(json.dumps(dict(measure="tv", n=n, degree=2, members=members, lattice_points=n ** 3, rays=N, tv_backward_ms=tv,
                              tv_backward_sigma_only_ms=tv_sigma_only, adam_step_ms=upd, march_backward_ms=round(bwd - zero, 3),
                              member_mask_ms=mask, tv_unique_GB=round(members * 28 * (4 + 16) / 1e9, 3))), flush=True)
        work = vol._replace(sigma=vol.sigma.clone(), coef=vol.coef.clone())
        thr = float(vol.sigma[vol.sigma > 0].median())
        in_place = med(lambda: ops.volume_prune(work.sigma, work.coef, thr), a.reps)
        copies = med(lambda: volume.prune(vol, thr), a.reps)
        pr = volume.prune(vol, thr)
        print(json.dumps(dict(measure="prune", n=n, degree=2, threshold=round(thr, 4), in_place_ms=in_place, with_copies_and_blocks_ms=copies,
                              active_before=members, active_after=int(volume.active(pr.sigma).numel()))), flush=True)
        del work, pr
        if n in a.upsample:
            del tuner, grad
            up_ms = med(lambda: ops.volume_upsample(vol.sigma, vol.coef), a.reps)
            whole = med(lambda: volume.upsample(vol), a.reps)
            m = 2 * n - 1
            print(json.dumps(dict(measure="upsample", n=n, to=m, degree=2, kernel_and_allocation_ms=up_ms, with_blocks_ms=whole,
                                  written_GB=round(m ** 3 * 112 / 1e9, 3), written_GB_per_s=round(m ** 3 * 112 / 1e6 / max(up_ms, 1e-9), 1))),
                  flush=True)
        del vol


if __name__ == "__main__":
    main()
