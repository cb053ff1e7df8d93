"""SH radiance volumes: the trained field baked onto a dense lattice and rendered without the network.

A Volume holds sigma on the lattice of NeRFModel.density_grid plus, per lattice point, the (degree + 1)^2 real spherical-harmonic
coefficients of the colour as a function of the viewing direction, and a block occupancy for the marcher.  ``NeRFModel.bake_volume``
makes one; ``render`` / ``render_views`` march rays through it with trilinear lookups on the device (one ray per lane), ``sample``
looks it up at points, ``save`` / ``load`` keep it as a plain ``.npz``.  The exact rules -- VA, VS, VO, VL and VR -- are in
include/nerf_hip.h.  An APPROXIMATE product of its own: a uniform-step estimator over interpolated values, not the renderer's coarse
+ fine composite; ``NeRFModel.render`` is untouched by it.

Everything runs on the device; a CPU tensor raises: there is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _abi, ops

ONE_BLOCK = 2**31 - 1  # a block edge that gives one block whatever the lattice


class Volume(NamedTuple):
    sigma: torch.Tensor    # [nx, ny, nz] fp32
    coef: torch.Tensor     # [nx, ny, nz, (degree + 1)^2, 3] fp32
    occ: torch.Tensor      # [bx, by, bz] uint8: blocks(sigma, block)
    lo: np.ndarray         # [3] fp32: lattice point (0, 0, 0)
    step: np.ndarray       # [3] fp32: the lattice step
    block: int             # cells per block edge
    degree: int            # 0, 1 or 2


def _on_device(t, what):
    t = torch.as_tensor(t)
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on a ROCm device (MI355X): move the input to 'cuda'; there is no CPU path")
    return t


def sh_dirs():
    """The 12 quadrature directions of rule VS (the icosahedron's vertices) -> [12, 3] fp32 numpy."""
    return np.asarray(_abi.volume_sh_table()[0], np.float32)


def blocks(sigma, block):
    """Rule VO: occ[bx, by, bz] uint8, 1 where some lattice point touched by a cell of the block has sigma > 0; ``block`` cells per
    edge (an int >= 1; ONE_BLOCK or anything >= every n - 1 gives a single block)."""
    return ops.volume_blocks(_on_device(sigma, "volume.blocks"), block)


def active(sigma):
    """Rule VA: the linear indices (int32, ascending) of the lattice points with a positive sigma in their clipped 3 x 3 x 3
    neighbourhood -- the points whose coefficients a lookup can read.  One host read of the count."""
    return ops.volume_active(_on_device(sigma, "volume.active"))


def with_block(vol, block):
    """vol with its occupancy rebuilt for another block edge (the arrays are shared)."""
    return vol._replace(occ=blocks(vol.sigma, block), block=min(int(block), ONE_BLOCK))


def sample(vol, points, dirs):
    """Rule VL: (sigma [M], rgb [M, 3]) of the volume at points [M, 3] along dirs [M, 3] (used as given, not renormalised): trilinear
    sigma, and the trilinear mean of the corners' SH colours clamped to [0, 1]; zeros outside the lattice."""
    _on_device(vol.sigma, "volume.sample")
    return ops.volume_sample(vol.sigma, vol.coef, vol.lo.tolist(), vol.step.tolist(), _on_device(points, "volume.sample"), torch.as_tensor(dirs))


def default_dt(vol):
    """Half the smallest lattice step, in fp32."""
    return float(np.float32(0.5) * np.float32(np.min(np.asarray(vol.step, np.float32))))


def render(vol, origins, dirs, tmin, tmax, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """Rule VR: rays (origins [N, 3], unit dirs [N, 3]) marched through the volume inside the window [tmin, tmax] (scalars or [N]) in
    steps of dt (default: half the smallest lattice step), ending a ray once its transmittance falls below t_stop (0: never)
    -> (rgb [N, 3], maps [N, 2] = (D, A) on render(maps=True)'s scale, steps [N, 2] int32 = (contributing, evaluated samples)).  Rays
    that miss the lattice get the background, zero maps and zero steps.  rgb, maps and steps[:, 0] do not depend on vol.block."""
    _on_device(vol.sigma, "volume.render")
    dt = default_dt(vol) if dt is None else float(dt)
    return ops.volume_render(vol.sigma, vol.coef, vol.occ, vol.block, vol.lo.tolist(), vol.step.tolist(), _on_device(origins, "volume.render"),
                             torch.as_tensor(dirs), tmin, tmax, dt, t_stop, background)


def render_views(vol, poses_bound17, K_inv, H, W, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """The volume seen from the cameras poses_bound17 [n, 17] along the renderer's own rays (mesh.camera_rays), each camera's window
    its own near / far (columns 15:17) -> (rgb [n, H, W, 3], maps [n, H, W, 2], steps [n, H, W, 2]).  The images feed
    metrics.image_metrics as they are."""
    from . import mesh

    dev = _on_device(vol.sigma, "volume.render_views").device
    pb = torch.as_tensor(poses_bound17).to(dev, torch.float32).reshape(-1, 17)
    n, H, W = int(pb.shape[0]), int(H), int(W)
    o, d = mesh.camera_rays(pb, K_inv, H, W, device=dev)
    near = pb[:, 15].repeat_interleave(H * W)
    far = pb[:, 16].repeat_interleave(H * W)
    rgb, maps, steps = render(vol, o, d, near, far, dt=dt, t_stop=t_stop, background=background)
    return rgb.view(n, H, W, 3), maps.view(n, H, W, 2), steps.view(n, H, W, 2)


def save(path, vol):
    """The volume as a plain ``.npz`` (numpy.savez: sigma, coef, occ, lo, step, block, degree)."""
    with open(path, "wb") as f:
        np.savez(f, sigma=vol.sigma.detach().cpu().numpy(), coef=vol.coef.detach().cpu().numpy(), occ=vol.occ.detach().cpu().numpy(),
                 lo=np.asarray(vol.lo, np.float32), step=np.asarray(vol.step, np.float32), block=np.int64(vol.block),
                 degree=np.int64(vol.degree))


def load(path, device="cuda"):
    """save()'s file -> a Volume on ``device`` with the saved bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("volume.load puts the volume on a ROCm device (MI355X): there is no CPU path")
    with np.load(path) as z:
        t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(dev)
        return Volume(t("sigma"), t("coef"), t("occ"), z["lo"].astype(np.float32).reshape(3), z["step"].astype(np.float32).reshape(3),
                      int(z["block"]), int(z["degree"]))
