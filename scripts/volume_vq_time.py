"""Times the vector-quantisation calls of compact SH radiance volumes on the analytic blob field of
scripts/mesh_band_time.py over [-3, 3]^3 at degree 2 (the field of scripts/volume_compact_time.py), medians of --reps HIP-event timings
after a warm-up:
  importance  volume.importance of --rays rays of the 400 x 400 camera of scripts/volume_compact_time.py beside volume.render of the
              same rays (fp16 rows)
  assign      one ops.volume_vq_assign over all rows at K = 256 and K = 4096, with the rate of the VALU operations it executes
              (per row and code 27 subtractions, 27 products, 26 sums and 1 compare = 81) against the fp32 vector peak, which
              counts an fma as two: operations that the rule forbids to fuse reach half of it at most (the *_of_unfused_peak figure)
  update      one ops.volume_vq_accumulate + ops.volume_vq_update at K = 4096
  decode      volume.dequantize of the K = 4096 form
  bytes       the FILE bytes (os.path.getsize of volume.save's output) dense / compact fp16 / VQ at keep_share 0 and 0.5, with and
              without prune_share 0.001 (K = 4096, --iters k-means iterations)
One JSON line per lattice size.
Usage: python scripts/volume_vq_time.py [--sizes 128 256] [--rays 65536] [--reps 7] [--iters 4] [--peak-tflops 157.3]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from nerf_tiny_amd import ops, volume  # noqa: E402
from mesh_band_time import blob_model  # noqa: E402


def median_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3)


def file_bytes(vol, tmp):
    path = os.path.join(tmp, "v.npz")
    volume.save(path, vol)
    n = os.path.getsize(path)
    os.remove(path)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="the fp32 vector peak the assign rate is stated against")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    blob = blob_model(dev)
    blob.eval()
    H = W = 400
    pose = torch.zeros(1, 17)
    pose[0, :15] = torch.tensor([[1.0, 0, 0, 0.3, 0], [0, 1.0, 0, 0.2, 0], [0, 0, 1.0, 2.6, 0]]).reshape(-1)
    pose[0, 15:] = torch.tensor([0.5, 5.5])
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -1.1 * W]]).t().contiguous()
    o, d = P.mesh.camera_rays(pose, K_inv, H, W, device=dev)
    pick = torch.randperm(H * W, generator=torch.Generator().manual_seed(0))[:a.rays].to(dev)
    o, d = o[pick].contiguous(), d[pick].contiguous()
    tmp = tempfile.mkdtemp()
    for n in a.sizes:
        dense = blob.bake_volume((-3.0,) * 3, (3.0,) * 3, n, degree=2, block=8)
        c16 = volume.pack(dense, "fp16")
        out = dict(n=n, degree=2, rows=int(c16.sigma.shape[0]), points=n ** 3, rays=int(o.shape[0]), reps=a.reps)
        out["file_bytes"] = dict(dense=file_bytes(dense, tmp), compact_fp16=file_bytes(c16, tmp))
        del dense
        out["render_ms"] = median_ms(lambda: volume.render(c16, o, d, 0.5, 5.5), a.reps)
        out["importance_ms"] = median_ms(lambda: volume.importance(c16, o, d, 0.5, 5.5), a.reps)
        imp, _ = volume.importance_views(c16, pose, K_inv, H, W)
        out["rows_with_importance"] = int((imp > 0).sum())
        rows = c16.coef[:, :27].to(torch.float32).contiguous()
        m = int(rows.shape[0])
        for K in (256, 4096):
            book, _ = volume.kmeans(rows, imp, K, 0)
            ms = median_ms(lambda: ops.volume_vq_assign(rows, book), a.reps)
            out[f"assign_K{K}_ms"] = ms
            out[f"assign_K{K}_tflops"] = round(81.0 * m * int(book.shape[0]) / (ms * 1e-3) / 1e12, 2)
            out[f"assign_K{K}_of_peak"] = round(out[f"assign_K{K}_tflops"] / a.peak_tflops, 3)
            out[f"assign_K{K}_of_unfused_peak"] = round(out[f"assign_K{K}_tflops"] / (0.5 * a.peak_tflops), 3)
        assign = ops.volume_vq_assign(rows, book)
        imax = int(imp.max())
        sums, counts = ops.volume_vq_accumulate(rows, imp, imax, assign, int(book.shape[0]))

        def update():
            sums.zero_(), counts.zero_()
            ops.volume_vq_accumulate(rows, imp, imax, assign, int(book.shape[0]), sums, counts)
            ops.volume_vq_update(book, sums, counts)

        out["accumulate_update_K4096_ms"] = median_ms(update, a.reps)
        del rows, book, sums, counts, assign
        for keep in (0.0, 0.5):
            for prune in (None, 0.001):
                vq = volume.quantize(c16, imp, K=4096, iters=a.iters, prune_share=prune, keep_share=keep)
                tag = f"vq_keep{keep:g}" + ("" if prune is None else f"_prune{prune:g}")
                out["file_bytes"][tag] = file_bytes(vq, tmp)
                out.setdefault("classes", {})[tag] = [int((vq.cls == k).sum()) for k in (0, 1, 2)]
                if keep == 0.0 and prune is None:
                    out["decode_ms"] = median_ms(lambda: volume.dequantize(vq), a.reps)
                del vq
        print(json.dumps(out), flush=True)
        del c16, imp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
