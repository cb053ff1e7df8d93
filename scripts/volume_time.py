"""Times the SH radiance volume on the 1,000-iteration analytic-sphere model of scripts/eval_modes.py:
  bake      NeRFModel.bake_volume at n^3 for degrees 0 and 2, split into its stages -- density grid, active list, lattice points +
            colour queries of the 12 directions, SH accumulation, block occupancy -- each stage between HIP events on buffers of its own
  frame     one image x image view: volume.render_views with blocks of 8 cells and with one block (the steps totals beside them), and
            NeRFModel.render of the same rays in exact fp32 and with bf16_mlp, alternating in one process after a warm-up, medians
  quality   PSNR / SSIM of the volume's frames against NeRFModel.render (exact fp32) of the same views: the held-out 64 x 64 views, and
            the image x image view above; per box and lattice
  blob      the same frame measurements on the analytic blob field of scripts/mesh_band_time.py (sigma = 100 max(0, cos(pi x) +
            cos(pi y) + cos(pi z) - 1.5): a blob of radius 0.55 at every even lattice point, 0 between them) over [-3, 3]^3, which holds
            everything the view sees between its near and far: a field with empty space, where the block skip has work to do
One JSON line per measurement.
Usage: python scripts/volume_time.py [--iters 1000] [--sizes 128 256] [--image 400] [--reps 5] [--boxes 1.5 3.0] [--sigma-min 0 1]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from nerf_tiny_amd import ops, volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402
from nerf_tiny_amd.nerf import grid_step  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def med(fn, reps):
    fn()
    return round(statistics.median(timed(fn)[0] for _ in range(reps)), 3)


def trained(iters, dev):
    H = W = 64
    scene = P.data.analytic_sphere_scene(n_pic=24, H=H, W=W, seed=5, device=dev)
    poses, imgs = scene.poses_bounds, scene.all_pix.view(24, H, W, 3)
    test_idx = np.arange(0, 24, 6)
    train_idx = np.setdiff1d(np.arange(24), test_idx)
    train = P.data.ArrayDataset(imgs[train_idx], poses[train_idx])
    test = P.data.ArrayDataset(imgs[test_idx], poses[test_idx])
    tmp = tempfile.mkdtemp()
    torch.manual_seed(0)
    run = P.NeRFRunner(gpu=0, img_dir="", results_path=tmp + "/", ckpt_path=tmp + "/ck/", low_res=1, total_iter=iters, batch_ray=4096,
                       learning=3e-4, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=64, n_fine=128, data_type="sync", step=10 ** 9,
                       decay_end=10 * iters, sched="EXP", continue_=False, datasets={"train": train, "val": train, "test": test},
                       log_every=max(iters // 4, 1), on_resample_fault="warn")
    run.trainer("train")
    run.model.eval()
    return run


def bake_stages(model, lo, hi, n, degree, reps):
    """the stages of NeRFModel.bake_volume, each timed alone (medians of reps after one warm-up)"""
    dev = next(model.parameters()).device
    shape = (n, n, n)
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    step = grid_step(lo32, hi32, shape)
    ps = model._params()
    out = {"grid_ms": med(lambda: model.density_grid(lo32, hi32, shape), reps)}
    sigma = model.density_grid(lo32, hi32, shape)
    out["active_ms"] = med(lambda: ops.volume_active(sigma), reps)
    index = ops.volume_active(sigma)
    out["active_points"] = int(index.numel())
    dirs = torch.from_numpy(volume.sh_dirs()).to(dev)
    pts = ops.volume_points(index, shape, lo32.tolist(), step.tolist())
    dk = [dirs[k].expand(pts.shape[0], 3).contiguous() for k in range(12)]
    ws = model._query_workspace(True, dev)

    def queries():
        ops.volume_points(index, shape, lo32.tolist(), step.tolist())
        for k in range(12):
            ops.query(ps, pts, dk[k], ws=ws)

    out["query_ms"] = med(queries, reps)
    out["query_Mpoints_per_s"] = round(12 * index.numel() / max(out["query_ms"], 1e-9) / 1e3, 1)
    coef = torch.zeros(*shape, (degree + 1) ** 2, 3, device=dev)
    rgb = ops.query(ps, pts, dk[0], ws=ws)[0]

    def accumulate():
        for k in range(12):
            ops.volume_sh_accumulate(coef, index, rgb, k)

    out["accumulate_ms"] = med(accumulate, reps)
    out["blocks_ms"] = med(lambda: ops.volume_blocks(sigma, 8), reps)
    del coef, pts, dk, rgb
    out["bake_ms"] = med(lambda: model.bake_volume(lo32, hi32, shape, degree=degree), max(reps // 2, 1))
    out["MiB"] = round(n ** 3 * (4 + 12 * (degree + 1) ** 2) / 2 ** 20, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--boxes", type=float, nargs="+", default=[1.5, 3.0], help="half edges of the baked boxes")
    ap.add_argument("--sigma-min", type=float, nargs="+", default=[0.0, 1.0])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    run = trained(a.iters, dev)
    model = run.model
    r = run.evaluate("disp", save=False)
    print(json.dumps({"model": f"analytic sphere, {a.iters} iterations", "heldout_psnr_db": round(r["psnr"], 3), "heldout_ssim": round(r["ssim"], 4)}),
          flush=True)
    box = a.boxes[0]
    for n in a.sizes:
        for degree in (0, 2):
            print(json.dumps(dict(measure="bake", n=n, degree=degree, box=box, **bake_stages(model, (-box,) * 3, (box,) * 3, n, degree, a.reps))),
                  flush=True)
    # one image x image view of the first held-out camera (the focal length scaled with the image)
    H = W = a.image
    pose = run.disp_rays.poses[:1]
    focal = float(run.focal) * H / run.height
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -focal]]).t().contiguous()
    row = torch.arange(H, device=dev).repeat_interleave(W)
    col = torch.arange(W, device=dev).repeat(H)
    per = pose.expand(H * W, 17).contiguous()
    model.batch_ray = run.batch_ray
    exact_frame = lambda: model.render(row, col, per, K_inv)[1]
    with torch.no_grad():
        model.bf16_mlp = False
        exact = exact_frame().view(H, W, 3)
        exact_ms = med(exact_frame, a.reps)
        model.bf16_mlp = True
        bf16 = exact_frame().view(H, W, 3)
        bf16_ms = med(exact_frame, a.reps)
        model.bf16_mlp = False
    m = P.metrics.image_metrics(bf16, exact)
    print(json.dumps(dict(measure="frame", path="model.render", image=[H, W], exact_fp32_ms=exact_ms, bf16_mlp_ms=bf16_ms,
                          bf16_vs_exact_psnr_db=round(m["psnr"], 3))), flush=True)
    blob = blob_model(dev)
    blob.batch_ray = run.batch_ray
    blob.eval()
    with torch.no_grad():
        blob_exact = blob.render(row, col, per, K_inv)[1].view(H, W, 3)
        blob_ms = med(lambda: blob.render(row, col, per, K_inv)[1], a.reps)
    for n in a.sizes:
        vol = blob.bake_volume((-3.0,) * 3, (3.0,) * 3, n, degree=2, block=8)
        out = dict(measure="blob", n=n, degree=2, box=3.0, image=[H, W], exact_fp32_ms=blob_ms, occupied_blocks=[int(vol.occ.sum()), int(vol.occ.numel())],
                   active_points=int((vol.coef[..., 0, 0] != 0).sum()))
        for name, v in (("block8", vol), ("block2", volume.with_block(vol, 2)), ("one_block", volume.with_block(vol, volume.ONE_BLOCK))):
            out[name + "_ms"] = med(lambda: volume.render_views(v, pose, K_inv, H, W), a.reps)
            rgb, _, steps = volume.render_views(v, pose, K_inv, H, W)
            out[name + "_steps"] = [int(steps[..., 0].sum()), int(steps[..., 1].sum())]
        m = P.metrics.image_metrics(rgb[0], blob_exact)
        out["vs_exact_psnr_db"], out["vs_exact_ssim"] = round(m["psnr"], 3), round(m["ssim"], 4)
        print(json.dumps(out), flush=True)
        del vol
    held = [run.render_view(i, "disp")[0] for i in range(run.disp_rays.pic_num)]
    for box in a.boxes:
        for n in a.sizes:
            for smin in a.sigma_min:
                vol = model.bake_volume((-box,) * 3, (box,) * 3, n, degree=2, sigma_min=smin, block=8)
                one = volume.with_block(vol, volume.ONE_BLOCK)
                out = dict(measure="frame", path="volume.render_views", n=n, degree=2, box=box, sigma_min=smin, image=[H, W],
                           occupied_blocks=[int(vol.occ.sum()), int(vol.occ.numel())])
                for name, v in (("block8", vol), ("one_block", one)):
                    out[name + "_ms"] = med(lambda: volume.render_views(v, pose, K_inv, H, W), a.reps)
                    rgb, _, steps = volume.render_views(v, pose, K_inv, H, W)
                    out[name + "_steps"] = [int(steps[..., 0].sum()), int(steps[..., 1].sum())]
                m = P.metrics.image_metrics(rgb[0], exact)
                out["vs_exact_psnr_db"], out["vs_exact_ssim"] = round(m["psnr"], 3), round(m["ssim"], 4)
                # the same with a white background: the scene's backdrop lies beyond the baked box
                rgbw = volume.render_views(vol, pose, K_inv, H, W, background=(1.0, 1.0, 1.0))[0]
                m = P.metrics.image_metrics(rgbw[0], exact)
                out["white_bg_psnr_db"], out["white_bg_ssim"] = round(m["psnr"], 3), round(m["ssim"], 4)
                ps, ss = [], []
                for i, ex in enumerate(held):
                    f = volume.render_views(vol, run.disp_rays.poses[i:i + 1], run.K_inv, run.height, run.width, background=(1.0, 1.0, 1.0))[0][0]
                    mm = P.metrics.image_metrics(f, ex)
                    ps.append(mm["psnr"])
                    ss.append(mm["ssim"])
                out["heldout_white_bg_psnr_db"], out["heldout_white_bg_ssim"] = round(float(np.mean(ps)), 3), round(float(np.mean(ss)), 4)
                print(json.dumps(out), flush=True)
                del vol, one


if __name__ == "__main__":
    main()
