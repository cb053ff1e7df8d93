"""Times narrow-band mesh extraction against the dense path: extract_mesh(color=False) with and without
band=R on the blob field sigma = 100 max(0, cos(pi x) + cos(pi y) + cos(pi z) - 1.5) over [-1, 1]^3 at level 30, alternating in one
process, HIP events after a warm-up of both, medians.  Also density_grid / density_band alone, and the banded call's launches without
the host reads between rounds (the counts of a first run replayed), which bounds what those reads cost.  One JSON line per size.
Usage: python scripts/mesh_band_time.py [--sizes 256 512] [--block 8] [--reps 5]
       --once: one warm-up and one timed call of each path per size, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from nerf_tiny_amd.nerf import grid_step  # noqa: E402

LO, HI, LEVEL, THR = (-1.0,) * 3, (1.0,) * 3, 30.0, 1.5


def blob_model(dev):
    torch.manual_seed(0)
    m = P.NeRFModel(64, 128, 8)
    w = m.state_dict()
    for i in range(8):
        w[f"network.point_layer.{i}.0.weight"].zero_()
        w[f"network.point_layer.{i}.0.bias"].zero_()
    w["network.sigma_layer.0.weight"].zero_()
    w["network.sigma_layer.0.bias"].zero_()
    for c in range(3):
        w["network.point_layer.0.0.weight"][0, 20 * c + 1] = 1.0  # cos(pi x_c)
    w["network.point_layer.0.0.bias"][0] = 3.0
    for i in range(1, 7):
        w[f"network.point_layer.{i}.0.weight"][0, 0] = 1.0
    w["network.point_layer.7.0.weight"][0, 0] = 100.0
    w["network.point_layer.7.0.bias"][0] = -100.0 * (3.0 + THR)
    w["network.sigma_layer.0.weight"][0, 0] = 1.0
    m.load_state_dict(w)
    return m.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def band_calls(model, n, block):
    """(begin(), grow(k), counts) of the banded grid's two C calls on buffers of their own."""
    ps, dev = model._params(), next(model.parameters()).device
    L, st = P._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    lo32 = np.float32(LO)
    step = grid_step(lo32, np.float32(HI), (n, n, n))
    ws = torch.empty(P._abi.band_ws_bytes(n, n, n, block), dtype=torch.uint8, device=dev)
    sigma = torch.empty(n, n, n, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    head = (P._abi.ptr_array(ps), P._abi.f32_array(lo32.tolist()), P._abi.f32_array(step.tolist()), n, n, n, block, LEVEL)
    tail = (sigma.data_ptr(), ws.data_ptr(), ws.numel(), counts.data_ptr(), st)
    keep = (ps, ws, sigma)  # (the closures own the buffers)
    return (lambda: P._abi.check(L.nerf_hip_band_begin(*head, *tail)), lambda k: (keep, P._abi.check(L.nerf_hip_band_grow(*head, k, *tail))),
            counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = blob_model(dev)
    reps, warm = (1, 1) if a.once else (a.reps, 1 if max(a.sizes) > 512 else 2)
    for n in a.sizes:
        dense = lambda: model.extract_mesh(LO, HI, n, LEVEL, color=False)
        band = lambda: model.extract_mesh(LO, HI, n, LEVEL, color=False, band=a.block)
        for _ in range(warm):
            d, b = dense(), band()
        same = all(torch.equal(x, y) for x, y in zip(d[:3], b[:3]))
        V, F = len(d.verts), len(d.faces)
        del d, b
        td, tb = [], []
        for _ in range(reps):  # alternating
            td.append(timed(dense)[0])
            tb.append(timed(band)[0])
        out = dict(n=n, block=a.block, V=V, F=F, same_mesh=same, dense_ms=round(statistics.median(td), 3),
                   band_ms=round(statistics.median(tb), 3))
        out["speedup"] = round(out["dense_ms"] / out["band_ms"], 2)
        if not a.once:
            tg = [timed(lambda: model.density_grid(LO, HI, n))[0] for _ in range(reps)]
            tq, info = [], None
            rounds = []
            for _ in range(reps):
                t, (_, info) = timed(lambda: model.density_band(LO, HI, n, LEVEL, block=a.block))
                tq.append(t)
            out.update(info=info, point_ratio=round(info["points_total"] / info["points_evaluated"], 2),
                       density_grid_ms=round(statistics.median(tg), 3), density_band_ms=round(statistics.median(tq), 3),
                       dense_Mpts_per_s=round(n ** 3 / statistics.median(tg) / 1e3, 1))
            # the per-round block counts, read once; then the same launches without the reads
            begin, grow, counts = band_calls(model, n, a.block)
            begin()
            while int(counts.cpu()[0]):
                rounds.append(int(counts.cpu()[0]))
                grow(rounds[-1])
            run = lambda: (begin(), [grow(k) for k in rounds])
            run()
            tr = [timed(run)[0] for _ in range(reps)]
            out.update(new_blocks_per_round=rounds, launches_only_ms=round(statistics.median(tr), 3))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
