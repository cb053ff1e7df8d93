"""Times mesh simplification by vertex clustering on a sphere field and a uniform random field (level 0.5) at
256^3 with cells of k = 2 and 4 lattice steps: nerf_hip_mesh_simplify_count + the 48-byte read of the counts + nerf_hip_mesh_simplify_emit
(mesh.simplify) -- beside, in the same process, marching-cubes count + emit, the component filter (label + ids + stats + compaction that
keeps the largest component) and the colour query of the same mesh, which are the yardsticks of section 3h-3: simplification pays
whenever it costs less than the colour (and field-normal) queries of the vertices it removes.  Also the area and the enclosed volume of
the mesh before and after (quality, reported and not gated).  HIP events after a warm-up, medians of --reps.  One JSON line per case.
Usage: python scripts/mesh_simplify_time.py [--reps 5] [--size 256] [--case sphere|random|all]"""
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
from mesh_time import sphere  # noqa: E402
from nerf_tiny_amd.nerf import simplify_lattice_of_grid  # noqa: E402


def median_ms(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(statistics.median(ts), 3)


def area_volume(verts, faces):
    v = verts.double()
    a, b, c = (v[faces[:, i].long()] for i in range(3))
    n = torch.cross(b - a, c - a, dim=1)
    return float(n.norm(dim=1).sum() / 2), float((a * torch.cross(b, c, dim=1)).sum() / 6)


def filter_largest(m):
    comps = P.mesh.components(m.faces, len(m.verts), m.verts)
    return P.mesh.filter_components(m, comps, P.mesh.select_components(comps, keep_largest=1))


def case(name, sigma, lo, step, level, reps, model, ks):
    out = dict(case=name, shape=list(sigma.shape))
    out["mc_count_emit_ms"] = median_ms(lambda: P.mesh.marching_cubes(sigma, level, lo, step), reps)
    verts, faces, normals = P.mesh.marching_cubes(sigma, level, lo, step)
    V, F = len(verts), len(faces)
    m = P.mesh.Mesh(verts, faces, normals, None)
    area, vol = area_volume(verts, faces)
    out.update(V=V, F=F, area=round(area, 6), volume=round(vol, 6))
    out["color_query_ms"] = median_ms(lambda: model.query(verts, -normals), reps)
    out["color_query_Mverts_per_s"] = round(V / out["color_query_ms"] / 1e3, 1)
    out["component_filter_ms"] = median_ms(lambda: filter_largest(m), reps)
    lo32 = np.asarray(lo, np.float32)
    for k in ks:
        cell, dims = simplify_lattice_of_grid(np.asarray(step, np.float32), tuple(sigma.shape), k)
        ws = torch.empty(P._abi.mesh_simplify_ws_bytes(V, F, dims), dtype=torch.uint8, device=verts.device)
        counts = torch.empty(6, dtype=torch.int64, device=verts.device)
        run = lambda: P.ops.mesh_simplify(verts, faces, normals, lo32.tolist(), cell.tolist(), dims, ws=ws, counts=counts)
        ms = median_ms(run, reps)
        sv, sf, sn, info = run()
        a1, v1 = area_volume(sv, sf)
        q1 = median_ms(lambda: model.query(sv, -sn), reps) if len(sv) else 0.0
        saved = round(out["color_query_ms"] - q1, 3)
        out[f"k{k}"] = dict(simplify_ms=ms, ws_MiB=round(ws.numel() / 2 ** 20, 1), V=info["verts_out"], F=info["faces_out"],
                            clusters=info["clusters"], degenerate=info["degenerate_faces"], duplicates=info["duplicate_faces"],
                            Mverts_in_per_s=round(V / ms / 1e3, 1), area=round(a1, 6), volume=round(v1, 6), color_query_ms=q1,
                            color_query_ms_saved=saved, pays_back=bool(ms < saved))
        del ws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--case", choices=["sphere", "random", "all"], default="all")
    ap.add_argument("--k", type=int, nargs="+", default=[2, 4])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    n = a.size
    if a.case in ("sphere", "all"):
        s, lo, step, level = sphere(n, dev)
        print(json.dumps(case(f"sphere{n}", s, lo, step, level, a.reps, model, a.k)), flush=True)
        del s
    if a.case in ("random", "all"):
        torch.manual_seed(0)
        r = torch.rand(n, n, n, device=dev)
        print(json.dumps(case(f"random{n}", r, [0.0] * 3, [1.0] * 3, 0.5, a.reps, model, a.k)), flush=True)


if __name__ == "__main__":
    main()
