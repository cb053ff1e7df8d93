"""What coarse-to-fine fine-tuning buys on the procedural scene: a runner trained for --iters iterations on
data.synthetic_scene, then NeRFRunner.bake_volume with the same total steps and rays per step for
  fixed        the field baked at --res^3 and fine-tuned there (the path of section 3h-13)
  up           baked at (--res / 2)^3, the lattice doubled to (--res - 1)^3 half way
  up+prune     the same with rule VP at --prune before the doubling
  up+prune+tv  the same with the TV prior at --tv (a choice, not a tuned value)
and the PSNR / SSIM of each result against the GROUND-TRUTH images, the active fraction (rule VA) and the empty-block fraction of the
baked and of the final volume.  The procedural scene's train, val and test splits are the same views: these are TRAINING views, not
held-out ones.  One JSON line per run.
Usage: python scripts/volume_refine_learn.py [--iters 300] [--res 64] [--finetune 200] [--batch 4096] [--prune 0.5] [--tv 1e-3]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402


def fractions(vol):
    return dict(active=round(int(P.volume.active(vol.sigma).numel()) / vol.sigma.numel(), 4),
                empty_blocks=round(1.0 - float(vol.occ.float().mean()), 4), shape=list(vol.sigma.shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--finetune", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--prune", type=float, default=0.5)
    ap.add_argument("--tv", type=float, default=1e-3)
    a = ap.parse_args()
    scene = P.data.synthetic_scene(n_pic=8, H=64, W=64)
    tmp = tempfile.mkdtemp()
    torch.manual_seed(0)
    run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=a.iters, batch_ray=4096,
                       learning=5e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                       decay_end=10 * a.iters, sched="EXP", continue_=False, datasets={"train": scene, "val": scene, "test": scene},
                       log_every=max(a.iters // 4, 1), on_resample_fault="warn")
    run.trainer("train")
    half = a.finetune // 2
    runs = [("fixed", a.res, {}),
            ("up", a.res // 2, dict(finetune_upsample=(half,))),
            ("up+prune", a.res // 2, dict(finetune_upsample=(half,), finetune_prune=a.prune)),
            ("up+prune+tv", a.res // 2, dict(finetune_upsample=(half,), finetune_prune=a.prune, finetune_tv=(a.tv, a.tv)))]
    for name, res, kw in runs:
        baked = fractions(run.bake_volume(res, degree=2, save=False))
        vol = run.bake_volume(res, degree=2, save=False, preview="train", finetune=a.finetune, finetune_batch=a.batch, **kw)
        ft = run.last_volume_finetune
        print(json.dumps(dict(run=name, views="training", baked_res=res, degree=2, finetune=a.finetune, batch=a.batch,
                              prune=kw.get("finetune_prune"), tv=kw.get("finetune_tv"), baked=baked, final=fractions(vol),
                              **{k: round(v, 5) if isinstance(v, float) else v for k, v in ft.items()})), flush=True)


if __name__ == "__main__":
    main()
