"""Times the edge topology, the smoothing steps and the face normals on a sphere field and a uniform random
field (level 0.5) at 256^3: the adjacency build (nerf_hip_mesh_edges_build), one step (nerf_hip_mesh_smooth_step), the normals
(nerf_hip_mesh_vertex_normals) and mesh.smooth(iterations=10) end to end -- beside, in the same process, marching-cubes count + emit,
the component filter that keeps the largest component and the colour query of the same mesh, the yardsticks of sections 3h-3 / 3h-4.
Reports the step's achieved bytes/s (the positions it reads and writes, the row offsets and the row entries with the neighbours'
positions they fetch) against the 8 TB/s of HBM, the workspace size, the topology counts and, for quality, the area and the enclosed
volume before and after 10 iterations (reported, not gated).  HIP events after a warm-up, medians of --reps.  One JSON line per case;
run one process per field (--case sphere, --case random).
Usage: python scripts/mesh_smooth_time.py [--reps 5] [--size 256] [--case sphere|random|all]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from mesh_simplify_time import area_volume, filter_largest, median_ms  # noqa: E402
from mesh_time import sphere  # noqa: E402

HBM_TBPS = 8.0


def case(name, sigma, lo, step, level, reps, model):
    out = dict(case=name, shape=list(sigma.shape))
    out["mc_count_emit_ms"] = median_ms(lambda: P.mesh.marching_cubes(sigma, level, lo, step), reps)
    verts, faces, normals = P.mesh.marching_cubes(sigma, level, lo, step)
    V, F = len(verts), len(faces)
    m = P.mesh.Mesh(verts, faces, normals, None)
    area, vol = area_volume(verts, faces)
    out.update(V=V, F=F, area=round(area, 6), volume=round(vol, 6))
    out["color_query_ms"] = median_ms(lambda: model.query(verts, -normals), reps)
    out["component_filter_ms"] = median_ms(lambda: filter_largest(m), reps)
    box_lo, scale = P.mesh.smooth_box(verts)
    ws = torch.empty(P._abi.mesh_edges_ws_bytes(V, F), dtype=torch.uint8, device=verts.device)
    counts = torch.empty(8, dtype=torch.int64, device=verts.device)
    out["ws_MiB"] = round(ws.numel() / 2 ** 20, 1)
    out["edges_build_ms"] = median_ms(lambda: P.ops.mesh_edges(faces, V, ws=ws, counts=counts), reps)
    degree, flags, _, _ = P.ops.mesh_edges(faces, V, ws=ws, counts=counts)
    topo = P.ops.mesh_edge_counts(counts.cpu().tolist(), V, F)
    out["topology"] = topo
    buf = torch.empty_like(verts)
    out["step_ms"] = median_ms(lambda: P.ops.mesh_smooth_step(verts, buf, F, box_lo.tolist(), float(scale), 0.5, flags, ws), reps)
    E = topo["edges"]
    # per vertex 12 B read + 12 B written + an 8 B offset + 4 B of flags; per directed edge a 4 B entry and the neighbour's 12 B
    step_bytes = V * 36 + 2 * E * 16
    out["step_GB"] = round(step_bytes / 1e9, 3)
    out["step_TBps"] = round(step_bytes / out["step_ms"] / 1e9, 3)
    out["step_fraction_of_hbm"] = round(out["step_TBps"] / HBM_TBPS, 3)
    out["normals_ms"] = median_ms(lambda: P.ops.mesh_vertex_normals(verts, faces, box_lo.tolist(), float(scale), ws=ws), reps)
    del ws, buf
    out["smooth10_ms"] = median_ms(lambda: P.mesh.smooth(m, 10), reps)
    sm, info = P.mesh.smooth(m, 10)
    a1, v1 = area_volume(sm.verts, sm.faces)
    out.update(area_after=round(a1, 6), volume_after=round(v1, 6), pinned=info["pinned"], scale=float(info["scale"]),
               Mverts_per_s_smooth10=round(V / out["smooth10_ms"] / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--case", choices=["sphere", "random", "all"], default="all")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    n = a.size
    if a.case in ("sphere", "all"):
        s, lo, step, level = sphere(n, dev)
        print(json.dumps(case(f"sphere{n}", s, lo, step, level, a.reps, model)), flush=True)
        del s
    if a.case in ("random", "all"):
        torch.manual_seed(0)
        r = torch.rand(n, n, n, device=dev)
        print(json.dumps(case(f"random{n}", r, [0.0] * 3, [1.0] * 3, 0.5, a.reps, model)), flush=True)


if __name__ == "__main__":
    main()
