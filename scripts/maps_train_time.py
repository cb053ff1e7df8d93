"""Times one autograd train step (forward + ray_loss + backward) with and without the differentiable depth / opacity maps (DESIGN.md
section 3l): `plain` = forward(maps=False), loss = ray_loss; `maps` = forward(maps=True), loss = ray_loss + sum(g * maps) with a non-zero
g, i.e. nerf_hip_forward_maps_train + nerf_hip_backward_maps.  The two alternate in one process, HIP events around each step, after a
warm-up of both; prints one JSON line per case (median ms of each and the ratio).  --sphere ITERS: also one seeded run of NeRFRunner on
the analytic sphere scene with and without MASK_WEIGHT, reporting held-out PSNR and the silhouette error of A_f (mean |A_f - alpha| over
the held-out views' pixels).
Usage: python scripts/maps_train_time.py [--reps 20] [--sphere 300]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

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


def step_times(kind, B, reps, dev):
    row, col, pb, K, Ct = O.lego_inputs(B, seed=3)
    row, col, pb, Ct = row.to(dev), col.to(dev), pb.float().to(dev), Ct.to(dev)
    m = P.NeRFModel(64, 128, B)
    m.load_state_dict(O.make_weights(4, sharp=True))
    m = m.to(dev)
    m.split_train, m.bf16_mlp = kind == "split_train", kind == "bf16"
    g = torch.randn(B, 4, generator=torch.Generator().manual_seed(1)).to(dev)

    def plain():
        Cc, Cf = m(row, col, pb, K)
        m.ray_loss(Cc, Cf, Ct).backward()

    def maps():
        Cc, Cf, M = m(row, col, pb, K, maps=True)
        (m.ray_loss(Cc, Cf, Ct) + (M * g).sum()).backward()

    for _ in range(3):
        timed(plain), timed(maps)
    t0, t1 = [], []
    for _ in range(reps):
        t0.append(timed(plain))
        t1.append(timed(maps))
    m0, m1 = statistics.median(t0), statistics.median(t1)
    return dict(case=f"{kind}_{B}", rays=B, plain_ms=round(m0, 4), maps_ms=round(m1, 4), ratio=round(m1 / m0, 4),
                plain_min_ms=round(min(t0), 4), maps_min_ms=round(min(t1), 4))


def sphere_run(iters, lam, dev):
    scene = P.data.analytic_sphere_scene(n_pic=24, H=48, W=48, seed=5, device=str(dev))
    held = P.data.analytic_sphere_scene(n_pic=27, H=48, W=48, seed=5, device=str(dev))  # (a ring of 27: views 24..26 lie between the training angles)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/res/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=iters, batch_ray=1024,
                           learning=5e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                           decay_end=10 ** 6, sched="EXP", datasets={"train": scene, "val": held, "test": held}, log_every=10 ** 9,
                           on_resample_fault="ignore", distributed=False, mask_weight=lam)
        run.trainer("train")
        r = run.evaluate("disp", views=[24, 25, 26], save=False)
        m = run.model
        errs = []
        with torch.no_grad():
            for v in (24, 25, 26):
                sl = slice(v * 48 * 48, (v + 1) * 48 * 48)
                rays = run.disp_rays
                idx = torch.arange(sl.start, sl.stop, device=dev)
                row, col, _, pb, _, alpha = rays.gather(idx, with_alpha=True)
                _, _, M = m.render(row, col, pb, run.K_inv, maps=True)
                errs.append(float((M[:, 3] - alpha).abs().mean()))
    return dict(case=f"sphere_mask_weight_{lam}", iters=iters, psnr=round(r["psnr"], 3), ssim=round(r["ssim"], 4),
                silhouette_err=round(sum(errs) / len(errs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sphere", type=int, default=0, metavar="ITERS")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for kind, B in (("fp32", 4096), ("fp32", 400), ("split_train", 400), ("bf16", 400), ("bf16", 4096)):
        print(json.dumps(step_times(kind, B, a.reps, dev)), flush=True)
    if a.sphere:
        for lam in (0.0, 0.1):
            print(json.dumps(sphere_run(a.sphere, lam, dev)), flush=True)


if __name__ == "__main__":
    main()
