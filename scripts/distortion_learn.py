"""What the distortion loss does to a short training run: the schedule of scripts/eval_modes.py on the analytic sphere
scene (20 training and 4 held-out views of 64x64, exact fp32) with DIST_WEIGHT 0 and 0.01, from the same initial weights.  Reported per
weight: held-out PSNR / SSIM (NeRFRunner.evaluate), the training batches' mean L_f per ray over the last 100 iterations (measured in both
runs by one more forward(maps=True, distortion=True) on the batch behind its optimizer step; the graph is dropped, the weights stay), and
the number of connected components of extract_mesh at one level (floaters show up as extra components).  Nothing is asserted; the table is
what comes out.  Prints one JSON line.
Usage (GPU box):  python scripts/distortion_learn.py [iterations] [batch_ray] [seed] [mesh_level]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402

WEIGHTS = (0.0, 0.01)
RES, BOX = 96, 1.5


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    LEVEL = float(sys.argv[4]) if len(sys.argv) > 4 else 10.0
    dev = torch.device("cuda:0")
    H = W = 64
    scene = P.data.analytic_sphere_scene(n_pic=24, H=H, W=W, seed=5, device=dev)
    poses, imgs = scene.poses_bounds, scene.all_pix.view(24, H, W, 3)
    test_idx = np.arange(0, 24, 6)
    train_idx = np.setdiff1d(np.arange(24), test_idx)
    train = P.data.ArrayDataset(imgs[train_idx], poses[train_idx])
    test = P.data.ArrayDataset(imgs[test_idx], poses[test_idx])
    out = {"scene": f"analytic sphere, {len(train_idx)} train / {len(test_idx)} held-out views of {H}x{W}, {batch}-ray batches, 64+128 samples",
           "iterations": iters, "seed": seed, "mesh": f"level {LEVEL}, {RES}^3 over [-{BOX}, {BOX}]^3", "dist_weight": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for lam in WEIGHTS:
            torch.manual_seed(seed)  # the same initial weights for both runs
            run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=iters, batch_ray=batch,
                               learning=3e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                               decay_end=10 * iters, sched="EXP", continue_=False, datasets={"train": train, "val": train, "test": test},
                               log_every=max(iters // 4, 1), on_resample_fault="warn", dist_weight=lam)
            # the mean L_f of the batches of the last 100 iterations: the runner's forward / train_step are wrapped to remember the batch,
            # the optimizer's step to look at it once more
            model, seen, last, steps = run.model, [], {}, [0]
            fwd, train_step, opt_step = model.forward, model.train_step, run.optimizer.step

            def forward(row, col, pb, K, **k):
                last["batch"] = (row, col, pb, K)
                return fwd(row, col, pb, K, **k)

            def one_call_step(row, col, pb, K, Ct):
                last["batch"] = (row, col, pb, K)
                return train_step(row, col, pb, K, Ct)

            def observed_step(*a, **k):
                r = opt_step(*a, **k)
                steps[0] += 1
                if steps[0] > iters - 100:
                    seen.append(float(fwd(*last["batch"], maps=True, distortion=True)[3][:, 1].detach().mean()))
                return r

            model.forward, model.train_step, run.optimizer.step = forward, one_call_step, observed_step
            run.trainer("train")
            model.forward, model.train_step, run.optimizer.step = fwd, train_step, opt_step
            r = run.evaluate("disp", save=False)
            mesh = model.extract_mesh((-BOX,) * 3, (BOX,) * 3, RES, LEVEL, color=False)
            comps = P.mesh.components(mesh.faces, len(mesh.verts))
            n_comp = int((comps.n_faces > 0).sum())
            out["dist_weight"][str(lam)] = {"psnr_db": round(r["psnr"], 3), "ssim": round(r["ssim"], 5),
                                            "mean_L_f_last_100": round(float(np.mean(seen)), 6),
                                            "mesh_components": n_comp, "mesh_faces": int(len(mesh.faces))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
