"""Times fine-tuning the vector-quantised SH radiance volume beside fine-tuning its dequantised compact form
on the analytic blob field of scripts/mesh_band_time.py baked over [-3, 3]^3 at degree 2, with the 400 x 400 camera of
scripts/volume_compact_train_time.py (importance from the whole image, batches of --rays random pixels, windows 0.5 .. 5.5).  Per
lattice size and K, HIP-event medians of --reps calls after a warm-up round, rates of 0 (the volume stays what the first call timed):
  step          VQFinetuner.step and CompactFinetuner.step on dequantize(vq), TAKING TURNS in one process
  reduce        ops.volume_vq_grad_reduce alone, the rows' accumulators refilled with ones before every call (outside the timing)
  update        ops.volume_vq_adam_step alone / ops.volume_compact_adam_step alone
  expand        ops.volume_vq_expand alone
and the rise of torch.cuda.max_memory_allocated over constructing each tuner and taking one step, beside what the layouts predict.
Nothing is gated.  One JSON line per (size, K).
Usage: python scripts/volume_vq_finetune_time.py [--sizes 128 256] [--codes 256 4096] [--rays 4096] [--reps 7] [--prune 0.001|none] [--keep 0.0]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402,F401
from nerf_tiny_amd import mesh, ops, volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def turns(fns, reps, before=None):
    """the functions' times, taken in turn (one call of each per round) after a warm-up round -> {name: median ms}"""
    for fn in fns.values():
        if before:
            before()
        fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            if before:
                before()
            ms[k].append(timed(fn))
    return {k: round(statistics.median(x), 3) for k, x in ms.items()}


def peak_of(make, step, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    tuner = make()
    step(tuner)
    torch.cuda.synchronize(dev)
    return int(torch.cuda.max_memory_allocated(dev) - before), tuner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--codes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--vq-iters", type=int, default=2)
    ap.add_argument("--prune", type=lambda x: None if x.lower() == "none" else float(x), default=0.001,
                    help="quantize's prune_share; 'none' prunes nothing, so every row the one view does not see is CODED")
    ap.add_argument("--keep", type=float, default=0.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    blob = blob_model(dev)
    blob.eval()
    H = W = a.image
    pose = torch.zeros(1, 17)
    pose[0, :15] = torch.tensor([[1.0, 0, 0, 0.3, 0], [0, 1.0, 0, 0.2, 0], [0, 0, 1.0, 2.6, 0]]).reshape(-1)   # looks down -z from z = 2.6
    pose[0, 15:] = torch.tensor([0.5, 5.5])
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -1.1 * W]]).t().contiguous()
    o_all, d_all = mesh.camera_rays(pose, K_inv, H, W, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    idx = torch.randint(H * W, (a.rays,), device=dev, generator=gen)
    o, d = o_all[idx].contiguous(), d_all[idx].contiguous()
    target = torch.full((a.rays, 3), 0.5, device=dev)
    N, W27 = a.rays, 27
    one_step = lambda t: t.step(o, d, 0.5, 5.5, target)
    for n in a.sizes:
        c16 = volume.pack(blob.bake_volume((-3.0,) * 3, (3.0,) * 3, n, degree=2, block=8), "fp16")
        torch.cuda.empty_cache()
        imp, _ = volume.importance_views(c16, pose, K_inv, H, W)
        rows = int(c16.sigma.shape[0])
        for K in a.codes:
            vq = volume.quantize(c16, imp, K=K, iters=a.vq_iters, prune_share=a.prune, keep_share=a.keep)
            counts = [int((vq.cls == k).sum()) for k in (0, 1, 2)]
            Kp = int(vq.codebook.shape[0])
            peak_vq, vt = peak_of(lambda: volume.VQFinetuner(vq, lr_sigma=0.0, lr_coef=0.0), one_step, dev)
            peak_c, ct = peak_of(lambda: volume.CompactFinetuner(volume.dequantize(vq), lr_sigma=0.0, lr_coef=0.0), one_step, dev)
            out = dict(n=n, degree=2, K=Kp, rays=N, rows=rows, pruned=counts[0], coded=counts[1], kept=counts[2],
                       largest_code=int(torch.diff(vt.offset).max()) if Kp else 0, empty_codes=int((torch.diff(vt.offset) == 0).sum()),
                       vq_tuner_peak_bytes=peak_vq, compact_tuner_peak_bytes=peak_c,
                       # rows: sigma 4 + fp32 row 108 + accumulators 8 + 216 + sigma moments 8 + rank 4 + member / kept_row 4;
                       # per kept row and per code: a master 108 + moments 216 (+ a code's accumulators 216); the slot lattice
                       vq_layout_bytes=rows * (4 + 108 + 224 + 8 + 4 + 4) + counts[2] * 324 + Kp * 540 + n ** 3 * 4,
                       compact_layout_bytes=rows * 564 + n ** 3 * 4)
            out.update({f"step_ms_{k}": v for k, v in turns(dict(vq=lambda: one_step(vt), compact=lambda: one_step(ct)), a.reps).items()})
            step = [vt.steps, ct.steps]

            def vq_update():
                step[0] += 1
                ops.volume_vq_adam_step(vt.cvol.sigma, vt.kept32, vt.kept_row, vt.codebook32, 2, vt.grad.acc_sigma, vt.grad.acc_coef, vt.acc_code,
                                        vt.m, vt.v, 1.0 / (3 * N), step[0], 0.0, 0.0)

            def compact_update():
                step[1] += 1
                ops.volume_compact_adam_step(ct.cvol.sigma, ct.cvol.coef, 2, ct.grad.acc_sigma, ct.grad.acc_coef, ct.m, ct.v, 1.0 / (3 * N), step[1],
                                             0.0, 0.0)

            out["reduce_ms"] = turns(dict(r=lambda: ops.volume_vq_grad_reduce(vt.grad.acc_coef, vt.offset, vt.member, vt.acc_code)), a.reps,
                                     before=lambda: vt.grad.acc_coef.fill_(1))["r"]
            vt.grad.acc_coef.zero_(), vt.acc_code.zero_()
            out.update({f"update_ms_{k}": v for k, v in turns(dict(vq=vq_update, compact=compact_update), a.reps).items()})
            out["expand_ms"] = turns(dict(e=lambda: ops.volume_vq_expand(vt.cls, vt.rank, vt.code, vt.kept32, vt.codebook32, 2, out=vt.cvol.coef,
                                                                         acc_coef_rows=vt.grad.acc_coef)), a.reps)["e"]
            out["reduce_update_expand_ms"] = round(out["reduce_ms"] + out["update_ms_vq"] + out["expand_ms"], 3)
            out["step_vq_over_compact"] = round(out["step_ms_vq"] / max(out["step_ms_compact"], 1e-9), 3)
            # what the bytes predict: per coded word the reduce reads and zeroes 16 B, the expand writes 4 B; the compact update moves
            # acc 8 + 8, x 4 + 4, m 4 + 4, v 4 + 4 = 40 B per word
            out["reduce_GBps"] = round(counts[1] * W27 * 16 / max(out["reduce_ms"], 1e-9) / 1e6, 1)
            out["expand_GBps"] = round(rows * W27 * 4 / max(out["expand_ms"], 1e-9) / 1e6, 1)
            out["compact_update_GBps"] = round(rows * (1 + W27) * 40 / max(out["update_ms_compact"], 1e-9) / 1e6, 1)
            print(json.dumps(out), flush=True)
            del vt, ct, vq
            torch.cuda.empty_cache()
        del c16, imp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
