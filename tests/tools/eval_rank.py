"""One rank of a tile-sharded NeRFRunner.evaluate(), started by tests/test_gpu_metrics.py in a FRESH child process: under
``python -m torch.distributed.run ... eval_rank.py OUT_DIR`` with NERF_DIST_BACKEND=gloo (every rank on the box's one GPU), or plainly
(``python eval_rank.py OUT_DIR``: the single-process runner the ranks are compared with).  No training: the initial weights (rank 0's,
broadcast).  Every rank writes OUT_DIR/rank<r>.pt = {result (None off rank 0), world, frame (view 1 as render_view gives it)}.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    out = sys.argv[1]
    if os.environ.get("NERF_DIST_BACKEND") == "gloo":
        os.environ["LOCAL_RANK"] = "0"  # every rank of the rehearsal on the box's one GPU

    import torch

    import nerf_tiny_amd as P

    torch.manual_seed(0)
    scene = P.data.synthetic_scene(n_pic=3, H=24, W=24, seed=4)
    kw = dict(gpu=0, img_dir="", results_path=os.path.join(out, "res") + "/", ckpt_path=os.path.join(out, "ck") + "/", low_res=1, total_iter=1,
              batch_ray=100, learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64, data_type="sync", step=1,
              decay_end=10000, sched="EXP", datasets={"train": scene, "val": scene, "test": scene}, log_every=1, on_resample_fault="warn")
    run = P.NeRFRunner(continue_=False, **kw)
    result = run.evaluate("disp", save=True)
    frame = run.render_view(1)[0].cpu()
    os.makedirs(out, exist_ok=True)
    if result is not None:
        result.pop("seconds")
    torch.save({"result": result, "world": run.world, "frame": frame}, os.path.join(out, f"rank{run.rank}.pt"))
    if run.distributed:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    print("EVAL-RANK-OK")


if __name__ == "__main__":
    main()
