"""Times TSDF fusion: mesh.tsdf_integrate's device call at n^3 with v synthetic views of a sphere of radius
0.6 (analytic depth and opacity along the renderer's own unit rays, H x W each), then, for scale, NeRFModel.density_grid at the same n
and NeRFModel.render(maps=True) of the same cameras on the blob field of scripts/mesh_band_time.py.  HIP events after a warm-up,
medians.  One JSON line per measurement; volume_GBps is the traffic of the two volumes (read and written once per launch of
TSDF_VIEWS_PER_LAUNCH views: 16 bytes per lattice point and launch) over the time, hbm_share that against 8 TB/s.
--color: instead, per size and view count, tsdf_integrate without and with colour fusion in the same run
(the sphere's analytic colour images), then mesh.tsdf_sample_color at the sphere mesh's vertices and at 1 M random points.
--masked: instead, at the first size, marching cubes' count + emit over the fused sphere unmasked and masked (valid = Wt > 0).
--label TEXT is copied into every line (which build of the library ran).
Usage: python scripts/mesh_tsdf_time.py [--sizes 256 512] [--views 8 64] [--image 400] [--reps 3] [--render-views 2]
                                        [--color | --masked] [--label TEXT]"""
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
from mesh_band_time import HI, LO, blob_model, timed  # noqa: E402
from mesh_raycast_time import k_inv, look_at  # noqa: E402

RADIUS = 0.6
HBM_BYTES_PER_S = 8e12


def cameras(n, dist=2.5):
    """n cameras on a Fibonacci sphere of radius dist, looking at the origin"""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    d = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    return np.stack([look_at(v * dist, near=1.0, far=4.0) for v in d])


def sphere_images(poses, K, H, W, dev):
    """-> depth, opacity [n, H, W] fp32 on the device: the sphere along the unit rays of mesh.camera_rays, in fp64"""
    o, u = P.mesh.camera_rays(poses, K, H, W, device=dev)
    o, u = o.double(), u.double()
    b = (o * u).sum(1)
    disc = b * b - ((o * o).sum(1) - RADIUS * RADIUS)
    hit = disc > 0
    t = torch.where(hit, -b - torch.sqrt(disc.clamp_min(0.0)), torch.full_like(b, float("inf")))
    n = poses.shape[0]
    return t.float().view(n, H, W), hit.float().view(n, H, W)


def sphere_colors(poses, K, H, W, dev):
    """-> rgb [n, H, W, 3] fp32 on the device: 0.5 + 0.5 * hit / |hit| where the pixel's ray meets the sphere, 0 elsewhere"""
    o, u = P.mesh.camera_rays(poses, K, H, W, device=dev)
    o, u = o.double(), u.double()
    b = (o * u).sum(1)
    disc = b * b - ((o * o).sum(1) - RADIUS * RADIUS)
    hit = o + (-b - torch.sqrt(disc.clamp_min(0.0)))[:, None] * u
    col = 0.5 + 0.5 * hit / hit.norm(dim=1, keepdim=True)
    return torch.where((disc > 0)[:, None], col, torch.zeros_like(col)).float().view(poses.shape[0], H, W, 3)


def time_color(a, dev, K, H, W, lo32, hi32):
    """--color: the colourless call and the colour call on the same inputs, then the sampler"""
    C = step = None
    for v in a.views:
        poses = torch.from_numpy(cameras(v)).to(dev)
        depth, opacity = sphere_images(poses, K, H, W, dev)
        rgb = sphere_colors(poses, K, H, W, dev)
        cams = [P.mesh.camera_q(p, K) for p in poses.cpu()]
        cam_o, Q = [c.tolist() for _, c in cams], [q.reshape(-1).tolist() for q, _ in cams]
        for n in a.sizes:
            step = P.nerf.grid_step(lo32, hi32, (n,) * 3)
            trunc = P.mesh.tsdf_trunc(step)
            T, Wt = P.mesh.tsdf_volume(n, dev)
            C = P.mesh.tsdf_color_volume(n, dev)
            args = (T, Wt, lo32.tolist(), step.tolist(), depth, opacity, cam_o, Q, trunc)
            plain = med(lambda: P.ops.tsdf_integrate(*args), a.reps)
            color = med(lambda: P.ops.tsdf_integrate(*args, rgb=rgb, color=C), a.reps)
            T.zero_(), Wt.zero_(), C.zero_()
            P.ops.tsdf_integrate(*args, rgb=rgb, color=C)
            print(json.dumps(dict(label=a.label, tsdf_integrate=n, views=v, image=[H, W], plain_ms=plain, color_ms=color,
                                  ratio=round(color / plain, 3), observed=int((Wt > 0).sum()), coloured=int((C[..., 3] > 0).sum()))), flush=True)
            if v == a.views[-1] and n == a.sizes[0]:
                verts = P.mesh.marching_cubes(P.mesh.tsdf_grid(T, Wt), 0.0, lo32, step)[0]
                pts = torch.rand(1_000_000, 3, device=dev) * 1.6 - 0.8
                for name, x in (("mesh vertices", verts), ("random points", pts)):
                    ms = med(lambda: P.mesh.tsdf_sample_color(C, lo32, step, x), a.reps)
                    ok = P.mesh.tsdf_sample_color(C, lo32, step, x)[1]
                    print(json.dumps(dict(label=a.label, tsdf_sample_color=n, points=name, M=len(x), ms=ms, valid=int(ok.sum()))), flush=True)
            del T, Wt, C


def time_masked(a, dev, K, H, W, lo32, hi32):
    """--masked: count + emit over the fused sphere, unmasked over the solid fill and masked over the empty one"""
    n, v = a.sizes[0], a.views[0]
    poses = torch.from_numpy(cameras(v)).to(dev)
    depth, opacity = sphere_images(poses, K, H, W, dev)
    step = P.nerf.grid_step(lo32, hi32, (n,) * 3)
    T, Wt = P.mesh.tsdf_volume(n, dev)
    P.mesh.tsdf_integrate(T, Wt, lo32, step, depth, poses, K, opacity=opacity)
    ws = torch.empty(P._abi.mesh_ws_bytes(n, n, n), dtype=torch.uint8, device=dev)
    solid, empty, valid = P.mesh.tsdf_grid(T, Wt, "solid"), P.mesh.tsdf_grid(T, Wt, "empty"), (Wt > 0).to(torch.uint8)
    # (marching_cubes reads the counts between its two calls: the time includes that synchronisation, equally for all three)
    for name, grid, m in (("unmasked, solid fill", solid, None), ("unmasked, empty fill", empty, None), ("masked, empty fill", empty, valid)):
        ms = med(lambda: P.mesh.marching_cubes(grid, 0.0, lo32, step, ws=ws, valid=m), a.reps)
        vv, ff, _ = P.mesh.marching_cubes(grid, 0.0, lo32, step, ws=ws, valid=m)
        print(json.dumps(dict(label=a.label, marching_cubes=n, views=v, grid=name, ms=ms, V=len(vv), F=len(ff))), flush=True)


def med(fn, reps):
    fn()
    return round(statistics.median(timed(fn)[0] for _ in range(reps)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--render-views", type=int, default=2, help="views rendered for the per-view render time")
    ap.add_argument("--color", action="store_true", help="time colour fusion against the colourless call, and the colour sampler")
    ap.add_argument("--masked", action="store_true", help="time masked against unmasked marching cubes over the fused sphere")
    ap.add_argument("--label", default="", help="copied into every line of --color / --masked")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = a.image
    K = k_inv(H, W)
    lo32, hi32 = np.asarray(LO, np.float32), np.asarray(HI, np.float32)
    if a.color or a.masked:
        (time_color if a.color else time_masked)(a, dev, K, H, W, lo32, hi32)
        return
    per_launch = P._abi.TSDF_VIEWS_PER_LAUNCH
    for v in a.views:
        poses = torch.from_numpy(cameras(v)).to(dev)
        depth, opacity = sphere_images(poses, K, H, W, dev)
        cams = [P.mesh.camera_q(p, K) for p in poses.cpu()]
        cam_o, Q = [c.tolist() for _, c in cams], [q.reshape(-1).tolist() for q, _ in cams]
        for n in a.sizes:
            step = P.nerf.grid_step(lo32, hi32, (n,) * 3)
            trunc = P.mesh.tsdf_trunc(step)
            T, Wt = P.mesh.tsdf_volume(n, dev)
            run = lambda: P.ops.tsdf_integrate(T, Wt, lo32.tolist(), step.tolist(), depth, opacity, cam_o, Q, trunc)
            ms = med(run, a.reps)
            launches = -(-v // per_launch)
            gbps = launches * n ** 3 * 16 / (ms * 1e-3) / 1e9
            T.zero_(), Wt.zero_()
            run()
            out = dict(tsdf_integrate=n, views=v, image=[H, W], ms=ms, launches=launches, Gproj_per_s=round(n ** 3 * v / ms / 1e6, 2),
                       volume_GBps=round(gbps, 1), hbm_share=round(gbps * 1e9 / HBM_BYTES_PER_S, 4), observed=int((Wt > 0).sum()), trunc=trunc)
            print(json.dumps(out), flush=True)
            del T, Wt
    model = blob_model(dev)
    for n in a.sizes:
        print(json.dumps(dict(density_grid=n, ms=med(lambda: model.density_grid(LO, HI, n), a.reps))), flush=True)
    poses = torch.from_numpy(cameras(max(a.views))).to(dev)[: a.render_views]
    row = torch.arange(H, device=dev).repeat_interleave(W)
    col = torch.arange(W, device=dev).repeat(H)
    render = lambda: [model.render(row, col, p.expand(H * W, 17), K, maps=True) for p in poses]
    ms = med(render, a.reps)
    print(json.dumps(dict(render_maps_views=len(poses), image=[H, W], ms=ms, ms_per_view=round(ms / len(poses), 3))), flush=True)
    n = a.sizes[0]
    fuse = lambda: model.fuse_depth((poses, K, H, W), LO, HI, n)
    print(json.dumps(dict(fuse_depth=n, views=len(poses), ms=med(fuse, a.reps))), flush=True)


if __name__ == "__main__":
    main()
