"""Times marching cubes on the device: count and emit separately (HIP events after warm-up), on a sphere field
at 256^3 and 512^3 and a uniform random field at 256^3, beside density_grid at the same resolutions and the colour query at the
vertices.  Prints one JSON line per case.  Usage: python scripts/mesh_time.py [--reps 20] [--sizes 256 512]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402


def events_ms(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def sphere(n, dev):
    h = 2.0 / (n - 1)
    x = torch.arange(n, device=dev, dtype=torch.float32) * h - 1.0
    r = torch.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    return (100 * torch.clamp(0.8 - r, min=0)).contiguous(), [-1.0] * 3, [h] * 3, 30.0


def mesh_case(name, sigma, lo, step, level, reps, model=None):
    dev = sigma.device
    nx, ny, nz = sigma.shape
    L, st = P._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(P._abi.mesh_ws_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    lo_a, step_a = P._abi.f32_array(lo), P._abi.f32_array(step)

    def count():
        P._abi.check(L.nerf_hip_mesh_count(sigma.data_ptr(), nx, ny, nz, level, ws.data_ptr(), ws.numel(), counts.data_ptr(), st))

    count()
    V, F = (int(c) for c in counts.cpu())
    verts, normals = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

    def emit():
        P._abi.check(L.nerf_hip_mesh_emit(sigma.data_ptr(), nx, ny, nz, lo_a, step_a, level, ws.data_ptr(), ws.numel(), verts.data_ptr(),
                                          normals.data_ptr(), faces.data_ptr(), V, F, st))

    t_count = events_ms(count, reps)
    t_both = events_ms(lambda: (count(), emit()), reps)
    N = nx * ny * nz
    # bytes each pass must move: sigma once per pass, the owners' offsets written and read back, the outputs
    b_count = 4 * N + 4 * V
    b_emit = 4 * N + 4 * V + 24 * V + 12 * F
    out = dict(case=name, shape=[nx, ny, nz], V=V, F=F, count_ms=round(t_count, 4), count_emit_ms=round(t_both, 4),
               emit_ms=round(t_both - t_count, 4), count_GBps=round(b_count / t_count / 1e6, 1),
               count_emit_GBps=round((b_count + b_emit) / t_both / 1e6, 1))
    if model is not None and V:
        out["color_query_ms"] = round(events_ms(lambda: model.query(verts, -normals), max(3, reps // 4)), 3)
        out["color_query_Mpts_per_s"] = round(V / out["color_query_ms"] / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    for n in a.sizes:
        s, lo, step, level = sphere(n, dev)
        print(json.dumps(mesh_case(f"sphere{n}", s, lo, step, level, a.reps, model)), flush=True)
        del s
        t = events_ms(lambda: model.density_grid((-1.5,) * 3, (1.5,) * 3, n), 2 if n >= 512 else 5)
        print(json.dumps(dict(case=f"density_grid{n}", ms=round(t, 2), Mpts_per_s=round(n ** 3 / t / 1e3, 1))), flush=True)
    r = torch.rand(256, 256, 256, device=dev)
    print(json.dumps(mesh_case("random256", r, [0.0] * 3, [1.0] * 3, 0.5, a.reps, model)), flush=True)


if __name__ == "__main__":
    main()
