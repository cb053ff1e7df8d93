"""What vector quantisation costs in image quality on the procedural scene of scripts/volume_finetune_learn.py (DESIGN.md section
3h-17): a runner trained for --iters iterations on data.synthetic_scene, its field baked at --res^3 degree 2 into the compact fp16
form, then NeRFRunner.bake_volume(vq=K) for each K: the PSNR / SSIM of the compact volume and of the dequantized volume against the
GROUND-TRUTH train views, and of the dequantized frames against the compact frames.  One JSON line per K.
Usage: python scripts/volume_vq_quality.py [--iters 300] [--res 64] [--codes 256 4096] [--vq-iters 10] [--prune 0.001] [--keep 0.0]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--codes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--vq-iters", type=int, default=10)
    ap.add_argument("--prune", type=float, default=None)
    ap.add_argument("--keep", type=float, default=0.0)
    a = ap.parse_args()
    scene = P.data.synthetic_scene(n_pic=8, H=64, W=64)
    tmp = tempfile.mkdtemp()
    torch.manual_seed(0)
    run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=a.iters, batch_ray=4096,
                       learning=5e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                       decay_end=10 * a.iters, sched="EXP", continue_=False, datasets={"train": scene, "val": scene, "test": scene},
                       log_every=max(a.iters // 4, 1), on_resample_fault="warn")
    run.trainer("train")
    rays = run.train_rays
    for K in a.codes:
        vol = run.bake_volume(a.res, degree=2, save=True, preview="train", compact="fp16", vq=K, vq_iters=a.vq_iters, vq_prune=a.prune,
                              vq_keep=a.keep)
        info = dict(run.last_volume_vq)
        dq = P.volume.dequantize(P.volume.load(info["path"]))
        ms = [P.metrics.image_metrics(P.volume.render_views(dq, rays.poses[i:i + 1], run.K_inv, rays.height, rays.width)[0],
                                      P.volume.render_views(vol, rays.poses[i:i + 1], run.K_inv, rays.height, rays.width)[0])
              for i in range(rays.pic_num)]
        info.update(vq_vs_compact_psnr_db=float(np.mean([float(m["psnr"][0]) for m in ms])),
                    vq_vs_compact_ssim=float(np.mean([float(m["ssim"][0]) for m in ms])),
                    file_bytes=os.path.getsize(info["path"]), compact_file_bytes=os.path.getsize(info["path"].replace(f"_vq{K}", "")))
        info.pop("path")
        print(json.dumps(dict(res=a.res, degree=2, iters=a.iters, vq_iters=a.vq_iters, prune=a.prune, keep=a.keep,
                              **{k: round(v, 5) if isinstance(v, float) else v for k, v in info.items()})), flush=True)


if __name__ == "__main__":
    main()
