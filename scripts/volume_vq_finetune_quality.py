"""What fine-tuning gives back of what vector quantisation cost, on the procedural scene of scripts/volume_vq_quality.py (DESIGN.md
section 3h-18): a runner trained for --iters iterations on data.synthetic_scene, its field baked at --res^3 degree 2 into the compact
fp16 form, then for each K NeRFRunner.bake_volume(vq=K, vq_finetune=--steps): PSNR / SSIM of the TRAIN views for
  compact        the compact fp16 volume
  vq             the VQ volume, untuned (dequantized)
  vq_ft          the VQ volume after --steps steps of --batch rays (volume.finetune_vq; dequantized)
  compact_ft     for scale: the compact volume given the same steps by volume.finetune_compact, written as fp16 rows
each against the ground-truth views and against the compact volume's own frames, with the bytes of each file.  The scene has NO
held-out views: every figure is on the views the tuning saw.  One JSON line per K.
Usage: python scripts/volume_vq_finetune_quality.py [--iters 300] [--res 64] [--codes 256 4096] [--steps 200] [--batch 4096] [--prune P] [--keep S]"""
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
    ap.add_argument("--codes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--vq-iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096)
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
    V = P.volume
    truth = rays.pixels.view(rays.pic_num, rays.height, rays.width, 3)
    frames = lambda v: torch.cat([V.render_views(v, rays.poses[i:i + 1], run.K_inv, rays.height, rays.width)[0] for i in range(rays.pic_num)])

    def scores(got, ref):
        m = P.metrics.image_metrics(got, ref)
        return round(float(m["psnr"].mean()), 3), round(float(m["ssim"].mean()), 5)

    compact_ft = None
    for K in a.codes:
        vol = run.bake_volume(a.res, degree=2, save=True, preview="train", compact="fp16", vq=K, vq_iters=a.vq_iters, vq_prune=a.prune,
                              vq_keep=a.keep, vq_finetune=a.steps, vq_finetune_batch=a.batch)
        info = dict(run.last_volume_vq)
        base = frames(vol)
        forms = dict(compact=(vol, info["path"].replace(f"_vq{K}", "")), vq=(V.dequantize(V.load(info["path"])), info["path"]),
                     vq_ft=(V.dequantize(V.load(info["finetune_path"])), info["finetune_path"]))
        if compact_ft is None:                           # the same for every K
            tuned, losses = V.finetune_compact(V.convert(vol, "fp32"), rays, run.K_inv, a.steps, batch=a.batch)
            path = tmp + "/compact_ft.npz"
            V.save(path, V.convert(tuned, "fp16"))
            compact_ft = (V.load(path), path, float(losses[0]), float(losses[-1]))
        forms["compact_ft"] = compact_ft[:2]
        out = dict(res=a.res, degree=2, iters=a.iters, K=info["K"], vq_iters=a.vq_iters, prune=a.prune, keep=a.keep, steps=a.steps, batch=a.batch,
                   pruned=info["pruned"], coded=info["coded"], kept=info["kept"], vq_first_loss=round(info["first_loss"], 6),
                   vq_last_loss=round(info["last_loss"], 6), compact_first_loss=round(compact_ft[2], 6), compact_last_loss=round(compact_ft[3], 6),
                   vq_finetune_seconds=round(info["finetune_seconds"], 2), views="train (the scene has no held-out views)")
        for name, (v, path) in forms.items():
            f = frames(v)
            out[f"{name}_vs_truth_psnr_db"], out[f"{name}_vs_truth_ssim"] = scores(f, truth)
            if name != "compact":
                out[f"{name}_vs_compact_psnr_db"], out[f"{name}_vs_compact_ssim"] = scores(f, base)
            out[f"{name}_file_bytes"] = os.path.getsize(path)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
