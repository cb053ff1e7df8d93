"""Times the compact SH radiance volume against the dense one on the analytic blob field of
scripts/mesh_band_time.py over [-3, 3]^3 at degree 2 (the field of scripts/volume_time.py's blob table), the 400 x 400 camera of
scripts/volume_grad_time.py (windows 0.5 .. 5.5):
  frame     volume.render_views of the dense, the compact fp32 and the compact fp16 form, alternating in one process after a warm-up,
            HIP-event medians, with blocks of 8 cells and with one block; the steps totals beside them
  pack      volume.pack (fp32, fp16) and volume.unpack, and the bytes of each form
  quality   PSNR / SSIM of the compact fp16 frame against the compact fp32 frame of the same view (metrics.image_metrics)
  big       NeRFModel.bake_volume(compact="fp16") at --big^3 (default 512), one frame from it, its bytes beside the dense form's
            (which is not allocated)
One JSON line per measurement.
Usage: python scripts/volume_compact_time.py [--sizes 128 256] [--big 512] [--image 400] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from nerf_tiny_amd import volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def frames(forms, pose, K_inv, H, W, reps):
    """the forms' frame times, taken in turn (one frame of each per round) after a warm-up round -> {name: median ms}"""
    for v in forms.values():
        volume.render_views(v, pose, K_inv, H, W)
    ms = {k: [] for k in forms}
    for _ in range(reps):
        for k, v in forms.items():
            ms[k].append(timed(lambda: volume.render_views(v, pose, K_inv, H, W))[0])
    return {k: round(statistics.median(x), 3) for k, x in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--big", type=int, default=512)
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    blob = blob_model(dev)
    blob.eval()
    H = W = a.image
    pose = torch.zeros(1, 17)
    pose[0, :15] = torch.tensor([[1.0, 0, 0, 0.3, 0], [0, 1.0, 0, 0.2, 0], [0, 0, 1.0, 2.6, 0]]).reshape(-1)   # looks down -z from z = 2.6
    pose[0, 15:] = torch.tensor([0.5, 5.5])
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -1.1 * W]]).t().contiguous()
    box = ((-3.0,) * 3, (3.0,) * 3)
    for n in a.sizes:
        dense = blob.bake_volume(*box, n, degree=2, block=8)
        c32, c16 = volume.pack(dense, "fp32"), volume.pack(dense, "fp16")
        out = dict(measure="frame", n=n, degree=2, image=[H, W], reps=a.reps, rows=int(c32.sigma.shape[0]), points=n ** 3,
                   bytes=dict(dense=volume.nbytes(dense), compact_fp32=volume.nbytes(c32), compact_fp16=volume.nbytes(c16)))
        for name, B in (("block8", 8), ("one_block", volume.ONE_BLOCK)):
            forms = {"dense": volume.with_block(dense, B), "compact_fp32": volume.with_block(c32, B), "compact_fp16": volume.with_block(c16, B)}
            out[name + "_ms"] = frames(forms, pose, K_inv, H, W, a.reps)
            steps = volume.render_views(forms["compact_fp16"], pose, K_inv, H, W)[2]
            out[name + "_steps"] = [int(steps[..., 0].sum()), int(steps[..., 1].sum())]
        f32 = volume.render_views(c32, pose, K_inv, H, W)[0][0]
        f16 = volume.render_views(c16, pose, K_inv, H, W)[0][0]
        fd = volume.render_views(dense, pose, K_inv, H, W)[0][0]
        m = P.metrics.image_metrics(f16, f32)
        out["fp16_vs_fp32_psnr_db"], out["fp16_vs_fp32_ssim"] = round(float(m["psnr"]), 3), round(float(m["ssim"]), 6)
        out["fp16_vs_fp32_max_abs"] = float((f16 - f32).abs().max())
        out["compact_fp32_equals_dense"] = bool(torch.equal(f32, fd))
        reps = a.reps
        out["pack_fp32_ms"] = round(statistics.median(timed(lambda: volume.pack(dense, "fp32"))[0] for _ in range(reps)), 3)
        out["pack_fp16_ms"] = round(statistics.median(timed(lambda: volume.pack(dense, "fp16"))[0] for _ in range(reps)), 3)
        del dense, forms, fd
        out["unpack_fp32_ms"] = round(statistics.median(timed(lambda: volume.unpack(c32))[0] for _ in range(reps)), 3)
        out["unpack_fp16_ms"] = round(statistics.median(timed(lambda: volume.unpack(c16))[0] for _ in range(reps)), 3)
        print(json.dumps(out), flush=True)
        del c32, c16
        torch.cuda.empty_cache()
    if a.big:
        n = a.big
        torch.cuda.reset_peak_memory_stats(dev)
        ms, big = timed(lambda: blob.bake_volume(*box, n, degree=2, block=8, compact="fp16"))
        out = dict(measure="big", n=n, degree=2, bake_ms=round(ms, 1), rows=int(big.sigma.shape[0]), points=n ** 3, bytes_compact_fp16=volume.nbytes(big),
                   bytes_dense_not_allocated=n ** 3 * 112 + int(big.occ.numel()), bake_peak_bytes=int(torch.cuda.max_memory_allocated(dev)))
        out["frame_ms"] = frames({"compact_fp16": big}, pose, K_inv, H, W, a.reps)["compact_fp16"]
        steps = volume.render_views(big, pose, K_inv, H, W)[2]
        out["steps"] = [int(steps[..., 0].sum()), int(steps[..., 1].sum())]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
