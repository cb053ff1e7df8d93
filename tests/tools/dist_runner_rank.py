"""One rank of a data-parallel NeRFRunner job with the distortion loss (DIST_WEIGHT > 0), started by tests/test_gpu_distortion.py under
``python -m torch.distributed.run`` in a FRESH child process, as tests/tools/mask_runner_rank.py is for the alpha-mask loss.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port P \
        tests/tools/dist_runner_rank.py OUT_DIR [--force-dist] [--iters K] [--dist-weight L] [--mask-weight L]

Without a launcher (plain ``python dist_runner_rank.py OUT_DIR``): the single-process runner, the thing the rank is compared with.
Rank 0 writes OUT_DIR/result.pt = {losses, weights (flat), ranks, distributed}.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dist-weight", type=float, default=0.05)
    ap.add_argument("--mask-weight", type=float, default=0.0)
    ap.add_argument("--force-dist", action="store_true", help="join a process group also as a single rank")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)

    import torch

    import nerf_tiny_amd as P

    scene = P.data.analytic_sphere_scene(n_pic=3, H=24, W=24, seed=4, device="cuda:0")
    torch.manual_seed(0)
    kw = dict(gpu=0, img_dir="", results_path=os.path.join(args.out, "res") + "/", ckpt_path=os.path.join(args.out, "ck") + "/", low_res=1,
              total_iter=args.iters, batch_ray=256, learning=1e-3, lr_gamma=0.1, lr_milestone=[10, 200], n_coarse=32, n_fine=64,
              data_type="sync", step=100, decay_end=10000, sched="EXP", datasets={"train": scene, "val": scene, "test": scene},
              log_every=1, on_resample_fault="warn", mask_weight=args.mask_weight, dist_weight=args.dist_weight)
    run = P.NeRFRunner(continue_=False, distributed=True if args.force_dist else None, **kw)
    losses = []
    if run.rank == 0:
        run.writer.add_scalar = lambda tag, v, it: losses.append((tag, float(v), it))
    assert run.trainer("train") == args.iters - 1
    if run.rank == 0:
        torch.save({"losses": [v for t, v, _ in losses if t.startswith("loss/")],
                    "weights": torch.cat([p.detach().reshape(-1).cpu() for p in run.model.network.parameters()]),
                    "ranks": run.world, "distributed": run.distributed}, os.path.join(args.out, "result.pt"))
        print("DIST-RUNNER-OK", run.world, flush=True)
    if run.distributed:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
