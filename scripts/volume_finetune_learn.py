"""What fine-tuning buys on the procedural scene: a runner trained for --iters iterations on
data.synthetic_scene, its field baked at --res^3 degree 2 over the default box, then NeRFRunner.bake_volume(finetune=...) against the
scene's own pixels; the PSNR / SSIM of the baked and of the fine-tuned volume against the GROUND-TRUTH images (the procedural scene's
train, val and test splits are the same views: these are training views), per pair of rates.  One JSON line per run.
Usage: python scripts/volume_finetune_learn.py [--iters 300] [--res 64] [--finetune 200] [--batch 4096] [--rates 0.1,0.01 0.03,0.003]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--finetune", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rates", nargs="+", default=["0.1,0.01", "0.03,0.003"])
    a = ap.parse_args()
    scene = P.data.synthetic_scene(n_pic=8, H=64, W=64)
    tmp = tempfile.mkdtemp()
    torch.manual_seed(0)
    run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=a.iters, batch_ray=4096,
                       learning=5e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                       decay_end=10 * a.iters, sched="EXP", continue_=False, datasets={"train": scene, "val": scene, "test": scene},
                       log_every=max(a.iters // 4, 1), on_resample_fault="warn")
    run.trainer("train")
    r = run.evaluate("disp", save=False)
    print(json.dumps({"model": f"procedural scene, {a.iters} iterations", "render_psnr_db": round(r["psnr"], 3), "render_ssim": round(r["ssim"], 4)}),
          flush=True)
    for rates in a.rates:
        lr_sigma, lr_coef = (float(x) for x in rates.split(","))
        run.bake_volume(a.res, degree=2, save=False, preview="train", finetune=a.finetune, finetune_batch=a.batch, finetune_lr=(lr_sigma, lr_coef))
        ft = run.last_volume_finetune
        print(json.dumps(dict(res=a.res, degree=2, finetune=a.finetune, batch=a.batch, lr_sigma=lr_sigma, lr_coef=lr_coef,
                              **{k: round(v, 5) if isinstance(v, float) else v for k, v in ft.items()})), flush=True)


if __name__ == "__main__":
    main()
