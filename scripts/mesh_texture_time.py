"""Times texture baking on the analytic sphere's marching-cubes mesh at n^3 and its simplify=k versions, with a
random-weight field as the shader (the field's cost does not depend on its weights): per mesh and atlas bound S, the chart
mesh.atlas_chart picks, then mesh.atlas_texels over the whole atlas alone, NeRFModel.query of the same W * H points alone,
NeRFModel.bake_texture (bands of about 2^20 texels: texels + query + the masked copy), 1 M mesh.sample_texture lookups and one
image x image mesh.render_texture (camera rays + ray cast + lookups; the cast alone beside it).  HIP events after a warm-up, medians.
One JSON line per mesh and atlas; "no chart fits" where the bound is too small for the face count.
Usage: python scripts/mesh_texture_time.py [--size 256] [--k 1 2 4] [--texture 1024 2048 4096] [--image 400] [--reps 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_tiny_amd as P  # noqa: E402
from mesh_raycast_time import cameras, k_inv, med  # noqa: E402
from mesh_time import sphere  # noqa: E402
from nerf_tiny_amd.nerf import simplify_lattice_of_grid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4], help="simplify= of each mesh (1: the marching-cubes mesh itself)")
    ap.add_argument("--texture", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.NeRFModel(64, 128, 8).to(dev)
    sigma, lo, step, level = sphere(a.size, dev)
    verts, faces, normals = P.mesh.marching_cubes(sigma, level, lo, step)
    full = P.mesh.Mesh(verts, faces, normals, None)
    lo32 = np.asarray(lo, np.float32)
    H = W = a.image
    K = k_inv(H, W)
    pose = torch.from_numpy(cameras(1)).to(dev)
    for k in a.k:
        m = full
        if k > 1:
            cell, dims = simplify_lattice_of_grid(np.asarray(step, np.float32), tuple(sigma.shape), k)
            m, _ = P.mesh.simplify(full, cell, lo32, dims)
        F = len(m.faces)
        h = P.mesh.build_raycast(m)
        cast_ms = med(lambda: P.mesh.render_depth(h, pose, K, H, W), a.reps)
        for S in a.texture:
            out = dict(mesh=f"sphere{a.size}", simplify=k, V=len(m.verts), F=F, texture=S)
            try:
                n = P.mesh.atlas_chart(F, S)
            except ValueError:
                print(json.dumps(dict(out, chart=None, note="no chart fits")), flush=True)
                continue
            _, _, _, tw, th = P.mesh.atlas_dims(F, n)
            T = tw * th
            out.update(chart=n, atlas=[tw, th], texels=T)
            out["atlas_texels_ms"] = med(lambda: P.mesh.atlas_texels(m, n), a.reps)
            p, d, mask = P.mesh.atlas_texels(m, n)
            out["owned_share"] = round(float(mask.float().mean()), 4)
            p, d = p.view(-1, 3), d.view(-1, 3)
            out["query_ms"] = med(lambda: model.query(p, d), a.reps)
            out["query_Mpoints_per_s"] = round(T / out["query_ms"] / 1e3, 1)
            del p, d, mask
            out["bake_ms"] = med(lambda: model.bake_texture(m, n), a.reps)
            out["texels_share_of_bake"] = round(out["atlas_texels_ms"] / out["bake_ms"], 4)
            tex = model.bake_texture(m, n)
            g = torch.Generator(device=dev).manual_seed(1)
            face = torch.randint(0, F, (1_000_000,), device=dev, generator=g, dtype=torch.int32)
            uv = torch.rand(1_000_000, 2, device=dev, generator=g, dtype=torch.float64)
            uv = torch.where(uv.sum(1, keepdim=True) > 1, 1 - uv, uv)
            out["sample_1M_ms"] = med(lambda: P.mesh.sample_texture(tex, face, uv), a.reps)
            out["render_texture_ms"] = med(lambda: P.mesh.render_texture(h, tex, pose, K, H, W), a.reps)
            out["render_depth_ms"] = cast_ms
            out["image"] = [H, W]
            out["hit_pixels"] = int(P.mesh.render_texture(h, tex, pose, K, H, W)[1].sum())
            print(json.dumps(out), flush=True)
            del tex


if __name__ == "__main__":
    main()
