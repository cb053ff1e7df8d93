"""Held-out quality of the training modes: the same short schedule on the analytic sphere scene (data.analytic_sphere_scene: 20 training
and 4 held-out views of 64x64) in exact fp32, with the split-fp32 train step (split_train) and with the bf16 MLP (bf16_mlp), from the
same initial weights; each scored by NeRFRunner.evaluate on the held-out views (PSNR, SSIM; the model's inference flags apply as in
display()).  Prints one JSON line.
Usage (GPU box):  python scripts/eval_modes.py [iterations] [batch_ray] [seed]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402

MODES = {"fp32": {}, "split_train": {"split_train": True}, "bf16_mlp": {"bf16_mlp": True}}


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    dev = torch.device("cuda:0")
    H = W = 64
    scene = P.data.analytic_sphere_scene(n_pic=24, H=H, W=W, seed=5, device=dev)
    poses, imgs = scene.poses_bounds, scene.all_pix.view(24, H, W, 3)
    test_idx = np.arange(0, 24, 6)
    train_idx = np.setdiff1d(np.arange(24), test_idx)
    train = P.data.ArrayDataset(imgs[train_idx], poses[train_idx])
    test = P.data.ArrayDataset(imgs[test_idx], poses[test_idx])
    out = {"scene": f"analytic sphere, {len(train_idx)} train / {len(test_idx)} held-out views of {H}x{W}, {batch}-ray batches, 64+128 samples",
           "iterations": iters, "seed": seed, "modes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, flags in MODES.items():
            torch.manual_seed(seed)  # the same initial weights for every mode
            run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=iters, batch_ray=batch,
                               learning=3e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                               decay_end=10 * iters, sched="EXP", continue_=False, datasets={"train": train, "val": train, "test": test},
                               log_every=max(iters // 4, 1), on_resample_fault="warn", **flags)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run.trainer("train")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r = run.evaluate("disp", save=False)
            out["modes"][name] = {"psnr_db": round(r["psnr"], 3), "ssim": round(r["ssim"], 5), "trainer_rays_per_s": round(iters * batch / dt, 1),
                                  "eval_seconds": round(r["seconds"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
