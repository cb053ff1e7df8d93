"""Times the mesh-component calls on a sphere field at 256^3 and a uniform random field at 256^3 (level 0.5):
labelling (the host-driven rounds with their 4-byte reads, and the same launches replayed without the reads), ids, stats and the
compaction that keeps the largest component -- beside, in the same process, marching-cubes count + emit and the colour query of the
same mesh, which is the yardstick: filtering pays whenever labelling + compaction cost less than the colour (and field-normal) queries
of the vertices they drop.  HIP events after a warm-up, medians of --reps.  One JSON line per case.
Usage: python scripts/mesh_components_time.py [--reps 5] [--size 256]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from mesh_time import sphere  # noqa: E402


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


def case(name, sigma, lo, step, level, reps, model):
    dev = sigma.device
    L, st = P._abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    out = dict(case=name, shape=list(sigma.shape))
    out["mc_count_emit_ms"] = median_ms(lambda: P.mesh.marching_cubes(sigma, level, lo, step), reps)
    verts, faces, normals = P.mesh.marching_cubes(sigma, level, lo, step)
    V, F = len(verts), len(faces)
    out.update(V=V, F=F)
    out["color_query_ms"] = median_ms(lambda: model.query(verts, -normals), reps)
    out["color_query_Mverts_per_s"] = round(V / out["color_query_ms"] / 1e3, 1)

    ws = torch.empty(P._abi.mesh_cc_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    vert_comp = torch.empty(V, dtype=torch.int32, device=dev)
    face_comp = torch.empty(F, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    rnd = lambda r: P._abi.check(L.nerf_hip_mesh_cc_round(faces.data_ptr(), V, F, r, ws.data_ptr(), ws.numel(), changed.data_ptr(), st))

    def label():
        r = 0
        while True:
            rnd(r)
            r += 1
            if int(changed.cpu()) == 0:
                return r

    rounds = label()
    out["rounds"] = rounds
    out["label_ms"] = median_ms(label, reps)
    out["label_launches_only_ms"] = median_ms(lambda: [rnd(r) for r in range(rounds)], reps)
    ids = lambda: P._abi.check(L.nerf_hip_mesh_cc_ids(faces.data_ptr(), V, F, ws.data_ptr(), ws.numel(), vert_comp.data_ptr(),
                                                      face_comp.data_ptr(), count.data_ptr(), st))
    # (ids reads the labels and leaves them as they are: it can be repeated on one labelling)
    out["ids_ms"] = median_ms(ids, reps)
    C = int(count.cpu())
    out["C"] = C
    n_verts = torch.empty(C, dtype=torch.int32, device=dev)
    n_faces = torch.empty(C, dtype=torch.int32, device=dev)
    lo_b, hi_b = torch.empty(C, 3, device=dev), torch.empty(C, 3, device=dev)
    out["stats_ms"] = median_ms(lambda: P._abi.check(L.nerf_hip_mesh_cc_stats(
        verts.data_ptr(), vert_comp.data_ptr(), face_comp.data_ptr(), V, F, n_verts.data_ptr(), n_faces.data_ptr(), lo_b.data_ptr(),
        hi_b.data_ptr(), C, st)), reps)
    comps = P.mesh.Components(vert_comp, face_comp, n_verts, n_faces, lo_b, hi_b, rounds)
    keep = P.mesh.select_components(comps, keep_largest=1)
    m = P.mesh.Mesh(verts, faces, normals, None)
    out["compact_ms"] = median_ms(lambda: P.mesh.filter_components(m, comps, keep), reps)
    kept = P.mesh.filter_components(m, comps, keep)
    out.update(kept_V=len(kept.verts), kept_F=len(kept.faces), largest_faces=int(n_faces.max()))
    out["filter_total_ms"] = round(out["label_ms"] + out["ids_ms"] + out["stats_ms"] + out["compact_ms"], 3)
    out["query_ms_of_dropped_verts"] = round(out["color_query_ms"] * (V - len(kept.verts)) / max(V, 1), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    n = a.size
    s, lo, step, level = sphere(n, dev)
    print(json.dumps(case(f"sphere{n}", s, lo, step, level, a.reps, model)), flush=True)
    del s
    r = torch.rand(n, n, n, device=dev)
    print(json.dumps(case(f"random{n}", r, [0.0] * 3, [1.0] * 3, 0.5, a.reps, model)), flush=True)


if __name__ == "__main__":
    main()
