"""Times fine-tuning the compact SH radiance volume beside the dense one on the analytic blob field of
scripts/mesh_band_time.py baked over [-3, 3]^3 at degree 2, with the 400 x 400 camera and the batches of scripts/volume_grad_time.py
(consecutive and random pixels, windows 0.5 .. 5.5).  Per lattice size and batch, the dense and the compact form TAKING TURNS in one
process, HIP-event medians after a warm-up round:
  forward    volume.render
  backward   volume.render_backward / compact_render_backward into zeroed accumulators (the zeroing is timed alone and subtracted)
  tv         volume.tv_backward with the tuner's list and mask / ops.volume_compact_tv_backward with the tuner's row -> point list
             (volume.compact_tv_backward would rebuild that list from the slot lattice on every call)
  update     ops.volume_adam_step / volume_compact_adam_step at rates of 0 (the volume stays what the forward timed)
  step       Finetuner.step / CompactFinetuner.step with the TV prior on, rates of 0
and, per size, the rise of torch.cuda.max_memory_allocated over constructing each tuner and taking one step.  --big (default 512) adds
a compact-only row: NeRFModel.bake_volume(compact="fp32") and the same quantities.  Nothing is gated.  One JSON line per measurement.
Usage: python scripts/volume_compact_train_time.py [--sizes 128 256] [--big 512] [--rays 4096 65536] [--image 400] [--reps 7]"""
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

TV = 1e-3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def turns(fns, reps):
    """the functions' times, taken in turn (one call of each per round) after a warm-up round -> {name: median ms}"""
    for fn in fns.values():
        fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return {k: round(statistics.median(x), 3) for k, x in ms.items()}


def peak_of(make, step, dev):
    """the allocator's peak over make() and one step(tuner), above what was allocated before -> (bytes, the tuner)"""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    tuner = make()
    step(tuner)
    torch.cuda.synchronize(dev)
    return int(torch.cuda.max_memory_allocated(dev) - before), tuner


def calls(tuner, o, d, g, target, N):
    """the five timed calls of one tuner of either form on one batch -> {quantity: fn}"""
    count = [0]
    if isinstance(tuner, volume.CompactFinetuner):
        vol, grad = tuner.cvol, tuner.grad
        back = lambda: volume.compact_render_backward(vol, grad, o, d, 0.5, 5.5, g)
        tv = lambda: ops.volume_compact_tv_backward(vol.slot, vol.sigma, vol.coef, vol.degree, tuner.point, TV, TV, 1e-9, grad.acc_sigma,
                                                    grad.acc_coef)     # (the tuner's cached list)

        def update():
            count[0] += 1
            ops.volume_compact_adam_step(vol.sigma, vol.coef, vol.degree, grad.acc_sigma, grad.acc_coef, tuner.m, tuner.v, 1.0 / (3 * N), count[0],
                                         0.0, 0.0)
    else:
        vol, grad = tuner.vol, tuner.grad
        back = lambda: volume.render_backward(vol, grad, o, d, 0.5, 5.5, g)
        tv = lambda: volume.tv_backward(vol, grad, tuner.index, tuner.member, TV, TV)

        def update():
            count[0] += 1
            ops.volume_adam_step(vol.sigma, vol.coef, tuner.index, grad.acc_sigma, grad.acc_coef, tuner.m, tuner.v, 1.0 / (3 * N), count[0], 0.0, 0.0)
    zero = lambda: (grad.acc_sigma.zero_(), grad.acc_coef.zero_())
    return dict(forward=lambda: volume.render(vol, o, d, 0.5, 5.5), zero=zero, backward_with_zeroing=lambda: (zero(), back()), tv=tv, update=update,
                step=lambda: tuner.step(o, d, 0.5, 5.5, target))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--big", type=int, default=512)
    ap.add_argument("--rays", type=int, nargs="+", default=[4096, 65536])
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
    o_all, d_all = mesh.camera_rays(pose, K_inv, H, W, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    box = ((-3.0,) * 3, (3.0,) * 3)
    rates = dict(lr_sigma=0.0, lr_coef=0.0, tv_sigma=TV, tv_coef=TV)
    o1, d1 = o_all[:4096].contiguous(), d_all[:4096].contiguous()
    one_step = lambda t: t.step(o1, d1, 0.5, 5.5, torch.full((4096, 3), 0.5, device=dev))
    for n in list(a.sizes) + ([a.big] if a.big else []):
        big = n == a.big and n not in a.sizes
        tuners = {}
        if big:
            cvol = blob.bake_volume(*box, n, degree=2, block=8, compact="fp32")
        else:
            dense = blob.bake_volume(*box, n, degree=2, block=8)
            cvol = volume.pack(dense)
            peak_dense, tuners["dense"] = peak_of(lambda: volume.Finetuner(dense, **rates), one_step, dev)
        peak_compact, tuners["compact"] = peak_of(lambda: volume.CompactFinetuner(cvol, **rates), one_step, dev)
        rows = int(cvol.sigma.shape[0])
        mem = dict(measure="memory", n=n, degree=2, rows=rows, points=n ** 3, compact_volume_bytes=volume.nbytes(cvol),
                   compact_tuner_peak_bytes=peak_compact, compact_layout_bytes=rows * 564 + n ** 3 * 4)
        if not big:
            mem.update(dense_volume_bytes=volume.nbytes(dense), dense_tuner_peak_bytes=peak_dense,
                       dense_layout_bytes=n ** 3 * (112 + 224 + 1) + rows * (224 + 4))
        print(json.dumps(mem), flush=True)
        for N in a.rays:
            for kind in ("one camera, consecutive pixels", "one camera, random pixels"):
                first = (H * W - N) // 2 if N <= H * W else 0
                idx = torch.arange(first, first + N, device=dev) % (H * W) if kind.endswith("consecutive pixels") else \
                    torch.randint(H * W, (N,), device=dev, generator=gen)
                o, d = o_all[idx].contiguous(), d_all[idx].contiguous()
                rgb, _, steps = volume.render(cvol, o, d, 0.5, 5.5)
                g = (2.0 * (rgb - 0.5)).contiguous()
                target = torch.full((N, 3), 0.5, device=dev)
                per = {name: calls(t, o, d, g, target, N) for name, t in tuners.items()}
                out = dict(measure="step", n=n, degree=2, rays=N, batch=kind, rows=rows, contributing=int(steps[:, 0].sum()),
                           looked_at=int(steps[:, 1].sum()))
                for q in ("forward", "zero", "backward_with_zeroing", "tv", "update", "step"):
                    ms = turns({name: c[q] for name, c in per.items()}, a.reps)
                    for name, x in ms.items():
                        out[f"{q}_ms_{name}"] = x
                for name in tuners:
                    out[f"backward_ms_{name}"] = round(out[f"backward_with_zeroing_ms_{name}"] - out[f"zero_ms_{name}"], 3)
                if not big:
                    for q in ("forward", "backward", "tv", "update", "step"):
                        out[f"{q}_compact_over_dense"] = round(out[f"{q}_ms_compact"] / max(out[f"{q}_ms_dense"], 1e-9), 2)
                print(json.dumps(out), flush=True)
        del tuners, cvol, per
        if not big:
            del dense
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
