"""Times the geometry evaluation on a sphere field and a uniform random field (level 0.5) at 256^3: the
measures (nerf_hip_mesh_measure), 1 M surface samples (nerf_hip_mesh_sample), the grid build over 1 M samples
(nerf_hip_points_grid_build), the nearest points at 1 M x 1 M with the queries in cell order and in their own order
(nerf_hip_points_nearest), and mesh.compare at 200 k samples end to end -- beside, in the same process, marching-cubes count + emit,
mesh.smooth(10) and the colour query of the same mesh, the yardsticks of sections 3h-3 ... 3h-6.  As the brute-force yardstick,
nearest at 100 k x 100 k against a chunked torch.cdist + min over the same points (fp32 distances there: a time, not a reference).
Reports the workspace sizes, the grid, and for quality the fixed-point area / volume beside the fp64 sums (reported, not gated).  HIP
events after a warm-up, medians of --reps.  One JSON line per case; run one process per field (--case sphere, --case random).
Usage: python scripts/mesh_distance_time.py [--reps 5] [--size 256] [--case sphere|random|all] [--samples 1000000]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from mesh_simplify_time import area_volume, median_ms  # noqa: E402
from mesh_time import sphere  # noqa: E402


def cdist_min(q, ref, chunk=4096):
    out = torch.empty(len(q), dtype=torch.int64, device=q.device)
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = torch.cdist(q[s:s + chunk], ref).argmin(1)
    return out


def case(name, sigma, lo, step, level, reps, model, n):
    out = dict(case=name, shape=list(sigma.shape), samples=n)
    out["mc_count_emit_ms"] = median_ms(lambda: P.mesh.marching_cubes(sigma, level, lo, step), reps)
    verts, faces, normals = P.mesh.marching_cubes(sigma, level, lo, step)
    V, F = len(verts), len(faces)
    m = P.mesh.Mesh(verts, faces, normals, None)
    out.update(V=V, F=F)
    out["color_query_ms"] = median_ms(lambda: model.query(verts, -normals), reps)
    out["smooth10_ms"] = median_ms(lambda: P.mesh.smooth(m, 10), reps)
    box_lo, scale = P.mesh.smooth_box(verts)
    box = (box_lo.tolist(), float(scale))
    out["measure_ms"] = median_ms(lambda: P.ops.mesh_measure(verts, faces, *box), reps)
    ms = P.mesh.measure(m)
    area, vol = area_volume(verts, faces)
    out.update(area=ms.area, volume=ms.volume, area_fp64=area, volume_fp64=vol, scale=float(scale))
    ws = torch.empty(max(P._abi.mesh_sample_ws_bytes(F), 256), dtype=torch.uint8, device=verts.device)
    out["sample_ws_MiB"] = round(ws.numel() / 2 ** 20, 2)
    out["sample_ms"] = median_ms(lambda: P.ops.mesh_sample(verts, faces, n, 0, *box, ws=ws), reps)
    pa, _ = P.mesh.sample_surface(m, n, 0)
    pb, _ = P.mesh.sample_surface(m, n, 1)
    glo, cell, dims = P.mesh.nearest_grid(pb)
    gws = torch.empty(P._abi.points_nearest_ws_bytes(n, n, dims), dtype=torch.uint8, device=verts.device)
    out.update(grid_dims=list(dims), grid_cell=float(cell), nearest_ws_MiB=round(gws.numel() / 2 ** 20, 1))
    out["grid_build_ms"] = median_ms(lambda: P.ops.points_grid(pb, glo.tolist(), float(cell), dims, n_query=n, ws=gws), reps)
    _, counts = P.ops.points_grid(pb, glo.tolist(), float(cell), dims, n_query=n, ws=gws)
    out["fullest_cell"] = int(counts.cpu()[1])
    for key, sort in (("nearest_sorted_ms", True), ("nearest_unsorted_ms", False)):
        out[key] = median_ms(lambda: P.ops.points_nearest(pa, n, glo.tolist(), float(cell), dims, gws, sort_queries=sort), reps)
    out["Mqueries_per_s_sorted"] = round(n / out["nearest_sorted_ms"] / 1e3, 1)
    del gws
    out["compare200k_ms"] = median_ms(lambda: P.mesh.compare(m, m, 200_000), reps)
    r = P.mesh.compare(m, m, 200_000)
    out.update(self_chamfer=r["chamfer"], clamped=r["clamped"])
    k = min(100_000, n)
    qa, rb = pa[:k].contiguous(), pb[:k].contiguous()
    out["nearest_100k_ms"] = median_ms(lambda: P.mesh.nearest(rb, qa), reps)
    out["cdist_min_100k_ms"] = median_ms(lambda: cdist_min(qa, rb), reps)
    idx, _ = P.mesh.nearest(rb, qa)
    out["cdist_agrees_on"] = float((cdist_min(qa, rb) == idx.long()).double().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--case", choices=["sphere", "random", "all"], default="all")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    n = a.size
    if a.case in ("sphere", "all"):
        s, lo, step, level = sphere(n, dev)
        print(json.dumps(case(f"sphere{n}", s, lo, step, level, a.reps, model, a.samples)), flush=True)
        del s
    if a.case in ("random", "all"):
        torch.manual_seed(0)
        r = torch.rand(n, n, n, device=dev)
        print(json.dumps(case(f"random{n}", r, [0.0] * 3, [1.0] * 3, 0.5, a.reps, model, a.samples)), flush=True)


if __name__ == "__main__":
    main()
