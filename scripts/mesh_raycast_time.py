"""Times the mesh ray caster on two meshes extracted at n^3: a sphere (sigma = 0.8 - |p| over [-1, 1]^3, level
0) and a random field (uniform noise, level 0.5 -- faces everywhere, the worst case for a grid).  Per mesh: the grid build
(mesh.build_raycast, its host reads included), 1 M camera rays closest hit over the default grid, rays against a (1, 1, 1) grid --
brute force through the same kernel, the baseline the grid must beat, at a ray count small enough to finish -- and mesh.visibility
from 8 cameras.  Then extract_mesh(color=False) on the blob field of scripts/mesh_band_time.py with and without visible=.  HIP events
after a warm-up, medians.  One JSON line per measurement.
Usage: python scripts/mesh_raycast_time.py [--size 256] [--random-size 256] [--reps 3] [--brute-rays 4096]"""
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
from mesh_band_time import HI, LEVEL, LO, blob_model, timed  # noqa: E402


def look_at(cam, target=(0.0, 0.0, 0.0), near=1.0, far=8.0):
    cam, target = np.asarray(cam, np.float64), np.asarray(target, np.float64)
    fwd = (target - cam) / np.linalg.norm(target - cam)
    right = np.cross(fwd, [0.0, 0.3, 1.0])
    right /= np.linalg.norm(right)
    pose = np.zeros((3, 5))
    pose[:, 0], pose[:, 1], pose[:, 2], pose[:, 3] = right, np.cross(right, fwd), fwd, cam
    return np.concatenate((pose.reshape(-1), [near, far])).astype(np.float32)


def cameras(n, dist=3.0):
    d = np.array([[1, 0.2, 0.3], [-0.6, 1, 0.1], [0.1, -0.7, 1], [-0.5, -0.6, -0.8], [0.9, 0.8, -0.4], [-1, 0.1, 0.5], [0.3, -1, -0.2], [0.2, 0.4, -1]])[:n]
    return np.stack([look_at(v / np.linalg.norm(v) * dist) for v in d])


def k_inv(H, W, fov=0.8):
    s = fov / H
    return torch.tensor([[s, 0, 0], [0, s, 0], [-s * H / 2, -s * W / 2, 1]], dtype=torch.float32)


def field(name, n, dev):
    if name == "sphere":
        g = torch.linspace(-1, 1, n, device=dev)
        x, y, z = torch.meshgrid(g, g, g, indexing="ij")
        return 0.8 - torch.sqrt(x * x + y * y + z * z), 0.0
    return torch.rand(n, n, n, device=dev, generator=torch.Generator(device=dev).manual_seed(16)), 0.5


def med(fn, reps):
    fn()
    return round(statistics.median(timed(fn)[0] for _ in range(reps)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--random-size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--brute-rays", type=int, default=4096)
    ap.add_argument("--image", type=int, default=512, help="H = W of the cameras (4 of them make the 1 M rays at 512)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = a.image
    K, poses = k_inv(H, W), torch.from_numpy(cameras(8)).to(dev)
    for name, n in (("sphere", a.size), ("random", a.random_size)):
        sigma, level = field(name, n, dev)
        step = 2.0 / (n - 1)
        v, f, _ = P.mesh.marching_cubes(sigma, level, (-1.0,) * 3, (step,) * 3)
        del sigma
        m = P.mesh.Mesh(v, f, None, None)
        out = dict(mesh=name, n=n, V=len(v), F=len(f))
        h = P.mesh.build_raycast(m)
        out.update(dims=h.dims, cell=float(h.cell), entries=h.entries, outside=h.outside, build_ms=med(lambda: P.mesh.build_raycast(m), a.reps))
        o, d = P.mesh.camera_rays(poses[:4], K, H, W)
        hit = P.mesh.raycast(h, o, d)[2] >= 0
        out.update(rays=len(o), rays_hit=int(hit.sum()), closest_ms=med(lambda: P.mesh.raycast(h, o, d), a.reps),
                   any_ms=med(lambda: P.mesh.raycast(h, o, d, any_hit=True), a.reps))
        out["Mrays_per_s"] = round(len(o) / out["closest_ms"] / 1e3, 2)
        hb = P.mesh.build_raycast(m, (h.lo, 1.0, (1, 1, 1)))
        pick = torch.linspace(0, len(o) - 1, a.brute_rays, device=dev).long()
        ob, db = o[pick].contiguous(), d[pick].contiguous()
        same = all(torch.equal(x, y) for x, y in zip(P.mesh.raycast(hb, ob, db), P.mesh.raycast(h, ob, db)))
        out.update(brute_rays=len(ob), brute_ms=med(lambda: P.mesh.raycast(hb, ob, db), 1), grid_same_rays_ms=med(lambda: P.mesh.raycast(h, ob, db), a.reps),
                   brute_equals_grid=same)
        seen, counts = P.mesh.visibility(m, poses, K, H, W)
        out.update(seen=int(seen.sum()), visibility_ms=med(lambda: P.mesh.visibility(m, poses, K, H, W), a.reps))
        print(json.dumps(out), flush=True)
        del h, hb, m, v, f
    model = blob_model(dev)
    plain = lambda: model.extract_mesh(LO, HI, a.size, LEVEL, color=False)
    vis = lambda: model.extract_mesh(LO, HI, a.size, LEVEL, color=False, visible=(poses, K, H, W))
    p, q = plain(), vis()
    print(json.dumps(dict(extract_mesh=a.size, F=len(p.faces), F_visible=len(q.faces), plain_ms=med(plain, a.reps), visible_ms=med(vis, a.reps))), flush=True)


if __name__ == "__main__":
    main()
