"""SH radiance volumes: the trained field baked onto a dense lattice and rendered without the network.

A Volume holds sigma on the lattice of NeRFModel.density_grid plus, per lattice point, the (degree + 1)^2 real spherical-harmonic
coefficients of the colour as a function of the viewing direction, and a block occupancy for the marcher.  ``NeRFModel.bake_volume``
makes one; ``render`` / ``render_views`` march rays through it with trilinear lookups on the device (one ray per lane), ``sample``
looks it up at points, ``save`` / ``load`` keep it as a plain ``.npz``.  The exact rules -- VA, VS, VO, VL and VR -- are in
include/nerf_hip.h.  An APPROXIMATE product of its own: a uniform-step estimator over interpolated values, not the renderer's coarse
+ fine composite; ``NeRFModel.render`` is untouched by it.

FINE-TUNING (rules VG and VU).  The bake only projects the field onto the lattice; ``render_backward`` is the
gradient of the march with respect to sigma and the coefficients, accumulated exactly in int64 fixed point (``grad_buffers``,
``gradients``), ``render_train`` is ``render`` with that gradient under torch.autograd, and ``Finetuner`` / ``finetune`` optimise the
baked values against ground-truth pixels with the support frozen: the active list of the volume as baked never grows.

COARSE TO FINE (rules VM, VT, VX and VP).  ``upsample`` doubles the lattice (2 n - 1 points per axis over the
same box), ``prune`` clears thin density and the coefficients nothing can read any more, ``member_mask`` / ``tv_backward`` add the
gradient of a total-variation prior over a level's active list to the same accumulators.  ``Finetuner(tv_sigma=, tv_coef=)`` applies
the prior every step and ``finetune(upsample_at=, prune=)`` trains level by level, each level with a fresh active list and fresh moments.

COMPACT VOLUMES (rule VC).  ``pack`` turns a Volume into a CompactVolume -- the rows of the active lattice
points behind an int32 slot lattice, the coefficients fp32 or fp16 --, ``unpack`` goes back, ``nbytes`` counts either form.
``sample``, ``render``, ``render_views``, ``default_dt``, ``with_block``, ``save`` and ``load`` take both forms; the compact march equals
the dense one bit for bit (fp16: the dense march of the rounded coefficients).  ``NeRFModel.bake_volume(compact=)`` bakes straight into
rows.  The training calls take the dense form only (TypeError): ``unpack`` is the way back to ``Finetuner``.

COMPACT TRAINING (rules VCG, VCU and VCT).  Calls of their own train the compact form in place:
``compact_grad_buffers`` / ``compact_render_backward`` / ``compact_tv_backward`` keep one int64 accumulator word per ROW word,
``CompactFinetuner`` / ``finetune_compact`` are ``Finetuner`` / ``finetune`` over fp32 rows with per-row moments.  Every result equals
the dense call's on ``unpack(cvol)``, gathered at the rows, bit for bit; only a refinement goes through a transient dense level.

VECTOR QUANTISATION (rules VI, VQ-A, VQ-U and VQ-D).  ``importance`` / ``importance_views`` score every row by
the rendering weight the training rays give it, ``vq_classes`` sorts the rows into pruned / coded / kept with exact integer
thresholds, ``kmeans`` clusters the coded rows on the device (reproducibly: fixed fp32 order, int64 sums), ``quantize`` puts the three
together into a VQVolume and ``dequantize`` decodes that back to a CompactVolume with fp16 rows.  The VQVolume is what ``save`` makes
SMALL (a bit mask, fp32 sigma, one class byte and at most one uint16 code per row, a codebook); on the device it is decoded before
anything reads it -- sample, render and the training calls refuse it (TypeError) -- so device memory is NOT reduced by it.

VQ FINE-TUNING (rules VQ-X, VQ-G and VQ-V).  ``VQFinetuner`` / ``finetune_vq`` are VQRF's fourth step: the
codebook, the kept rows and sigma of a VQVolume trained jointly against rays with the assignments frozen.  The march and its gradient
are the compact ones over fp32 rows expanded from the masters; the rows' int64 accumulators are summed per code, exactly, and one Adam
launch updates the three kinds of parameter.  ``VQFinetuner.volume()`` is a VQVolume again: the file stays as small as it was.

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


class CompactVolume(NamedTuple):
    slot: torch.Tensor     # [nx, ny, nz] int32: the row of the lattice point, -1 where it has none (rule VC)
    sigma: torch.Tensor    # [n] fp32: the active points' sigma, in the order of rule VA's list
    coef: torch.Tensor     # [n, 3 (degree + 1)^2] fp32, or [n, that rounded up to a multiple of 4] fp16 with +0 pad halves
    occ: torch.Tensor      # [bx, by, bz] uint8: blocks(the dense sigma, block)
    lo: np.ndarray         # [3] fp32
    step: np.ndarray       # [3] fp32
    block: int
    degree: int
    shape: tuple           # (nx, ny, nz)


_DTYPES = {"fp32": False, "fp16": True}


def _on_device(t, what):
    t = torch.as_tensor(t)
    if t.device.type != "cuda":
        raise RuntimeError(f"{what} runs only on a ROCm device (MI355X): move the input to 'cuda'; there is no CPU path")
    return t


def _no_vq(vol, what):
    """a VQVolume is a file form: nothing marches, samples or trains it"""
    if isinstance(vol, VQVolume):
        raise TypeError(f"{what} does not read a VQVolume: it is the small FILE form -- volume.dequantize(vq) gives the CompactVolume "
                        "(fp16 rows) that is sampled, rendered and trained; volume.VQFinetuner / finetune_vq train the quantised form "
                        "itself (the codebook, the kept rows and sigma)")
    return vol


def _dense_only(vol, what):
    _no_vq(vol, what)
    if isinstance(vol, CompactVolume):
        raise TypeError(f"{what} works on the dense volume.Volume: a CompactVolume is the deployment form -- volume.unpack(cvol) gives the "
                        "dense volume back")
    return vol


def _anchor(vol):
    """the tensor that says where a volume of either form lives"""
    return vol.slot if isinstance(vol, CompactVolume) else vol.sigma


def pack(vol, dtype="fp32"):
    """Rule VC: the dense ``vol`` as a CompactVolume -- active(vol.sigma) -> the slot lattice -> the rows, gathered on the device;
    dtype "fp32" keeps the coefficients' bits, "fp16" rounds them to nearest even (past 65504: +-inf).  occ and block are taken over.
    What the inactive points of ``vol`` hold is dropped: no lookup with a positive sigma can read it."""
    _dense_only(vol, "volume.pack")
    if dtype not in _DTYPES:
        raise ValueError(f"dtype={dtype!r}: 'fp32' or 'fp16'")
    _on_device(vol.sigma, "volume.pack")
    index = active(vol.sigma)
    shape = tuple(int(n) for n in vol.sigma.shape)
    slot = ops.volume_compact_slots(index, shape)
    sigma_rows, coef_rows = ops.volume_compact_pack(vol.sigma.detach(), vol.coef.detach(), index, _DTYPES[dtype])
    return CompactVolume(slot, sigma_rows, coef_rows, vol.occ, np.asarray(vol.lo, np.float32), np.asarray(vol.step, np.float32), vol.block,
                         vol.degree, shape)


def _row_points(cvol):
    """index[n] int32: the lattice point that holds row r (-1: none), from the slots that lie in [0, n)"""
    flat = cvol.slot.reshape(-1)
    n = int(cvol.sigma.shape[0])
    where = torch.nonzero((flat >= 0) & (flat < n)).reshape(-1)
    index = torch.full((n,), -1, dtype=torch.int32, device=flat.device)
    index[flat[where].long()] = where.to(torch.int32)
    return index


def unpack(cvol):
    """Rule VC: the dense Volume that holds the rows at their lattice points and +0 everywhere else (fp16 widened: exact).  For a
    packed volume the points with a slot, in lattice order, are the active list.  sample / render of the result equal sample / render
    of ``cvol`` bit for bit."""
    if not isinstance(cvol, CompactVolume):
        raise TypeError("volume.unpack takes a CompactVolume")
    _on_device(cvol.slot, "volume.unpack")
    sigma, coef = ops.volume_compact_unpack(cvol.sigma, cvol.coef, _row_points(cvol), cvol.shape, cvol.degree)
    return Volume(sigma, coef, cvol.occ, np.asarray(cvol.lo, np.float32), np.asarray(cvol.step, np.float32), cvol.block, cvol.degree)


def nbytes(vol):
    """The bytes of the volume's arrays (dense: sigma, coef, occ; compact: slot, the rows, occ; VQ: point, sigma, cls, code, kept,
    codebook -- its file is smaller still: save writes a bit mask of the lattice in place of point)."""
    if isinstance(vol, VQVolume):
        return sum(int(t.numel()) * t.element_size() for t in (vol.point, vol.sigma, vol.cls, vol.code, vol.kept, vol.codebook))
    ts = (vol.slot, vol.sigma, vol.coef, vol.occ) if isinstance(vol, CompactVolume) else (vol.sigma, vol.coef, vol.occ)
    return sum(int(t.numel()) * t.element_size() for t in ts)


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
    """vol with its occupancy rebuilt for another block edge (the arrays are shared).  A CompactVolume rebuilds it from a temporary
    dense sigma of 4 bytes per lattice point."""
    _no_vq(vol, "volume.with_block")
    if isinstance(vol, CompactVolume):
        _on_device(vol.slot, "volume.with_block")
        sigma, _ = ops.volume_compact_unpack(vol.sigma, None, _row_points(vol), vol.shape, vol.degree)
        return vol._replace(occ=blocks(sigma, block), block=min(int(block), ONE_BLOCK))
    return vol._replace(occ=blocks(vol.sigma, block), block=min(int(block), ONE_BLOCK))


def sample(vol, points, dirs):
    """Rule VL: (sigma [M], rgb [M, 3]) of the volume at points [M, 3] along dirs [M, 3] (used as given, not renormalised): trilinear
    sigma, and the trilinear mean of the corners' SH colours clamped to [0, 1]; zeros outside the lattice.  A CompactVolume is looked
    up through its slots (rule VC-L): the same bits as sample(unpack(vol), ...)."""
    _on_device(_anchor(_no_vq(vol, "volume.sample")), "volume.sample")
    if isinstance(vol, CompactVolume):
        return ops.volume_compact_sample(vol.slot, vol.sigma, vol.coef, vol.degree, vol.lo.tolist(), vol.step.tolist(),
                                         _on_device(points, "volume.sample"), torch.as_tensor(dirs))
    return ops.volume_sample(vol.sigma, vol.coef, vol.lo.tolist(), vol.step.tolist(), _on_device(points, "volume.sample"), torch.as_tensor(dirs))


def default_dt(vol):
    """Half the smallest lattice step, in fp32."""
    return float(np.float32(0.5) * np.float32(np.min(np.asarray(vol.step, np.float32))))


def render(vol, origins, dirs, tmin, tmax, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """Rule VR: rays (origins [N, 3], unit dirs [N, 3]) marched through the volume inside the window [tmin, tmax] (scalars or [N]) in
    steps of dt (default: half the smallest lattice step), ending a ray once its transmittance falls below t_stop (0: never)
    -> (rgb [N, 3], maps [N, 2] = (D, A) on render(maps=True)'s scale, steps [N, 2] int32 = (contributing, evaluated samples)).  Rays
    that miss the lattice get the background, zero maps and zero steps.  rgb, maps and steps[:, 0] do not depend on vol.block.  A
    CompactVolume is marched through its slots (rule VC-R): the same bits as render(unpack(vol), ...)."""
    _on_device(_anchor(_no_vq(vol, "volume.render")), "volume.render")
    dt = default_dt(vol) if dt is None else float(dt)
    if isinstance(vol, CompactVolume):
        return ops.volume_compact_render(vol.slot, vol.sigma, vol.coef, vol.degree, vol.occ, vol.block, vol.lo.tolist(), vol.step.tolist(),
                                         _on_device(origins, "volume.render"), torch.as_tensor(dirs), tmin, tmax, dt, t_stop, background)
    return ops.volume_render(vol.sigma, vol.coef, vol.occ, vol.block, vol.lo.tolist(), vol.step.tolist(), _on_device(origins, "volume.render"),
                             torch.as_tensor(dirs), tmin, tmax, dt, t_stop, background)


def render_views(vol, poses_bound17, K_inv, H, W, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """The volume seen from the cameras poses_bound17 [n, 17] along the renderer's own rays (mesh.camera_rays), each camera's window
    its own near / far (columns 15:17) -> (rgb [n, H, W, 3], maps [n, H, W, 2], steps [n, H, W, 2]).  The images feed
    metrics.image_metrics as they are."""
    from . import mesh

    dev = _on_device(_anchor(_no_vq(vol, "volume.render_views")), "volume.render_views").device
    pb = torch.as_tensor(poses_bound17).to(dev, torch.float32).reshape(-1, 17)
    n, H, W = int(pb.shape[0]), int(H), int(W)
    o, d = mesh.camera_rays(pb, K_inv, H, W, device=dev)
    near = pb[:, 15].repeat_interleave(H * W)
    far = pb[:, 16].repeat_interleave(H * W)
    rgb, maps, steps = render(vol, o, d, near, far, dt=dt, t_stop=t_stop, background=background)
    return rgb.view(n, H, W, 3), maps.view(n, H, W, 2), steps.view(n, H, W, 2)


class VolumeGrad(NamedTuple):
    acc_sigma: torch.Tensor   # [nx, ny, nz] int64: sums of llrint(x 2^40)
    acc_coef: torch.Tensor    # [nx, ny, nz, (degree + 1)^2, 3] int64


def grad_buffers(vol):
    """Zeroed accumulators of rule VG for ``vol``: 8 bytes per parameter."""
    _dense_only(vol, "volume.grad_buffers")
    _on_device(vol.sigma, "volume.grad_buffers")
    return VolumeGrad(torch.zeros(vol.sigma.shape, dtype=torch.int64, device=vol.sigma.device),
                      torch.zeros(vol.coef.shape, dtype=torch.int64, device=vol.sigma.device))


def render_backward(vol, grad, origins, dirs, tmin, tmax, g_rgb, g_maps=None, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """Rule VG: the gradient of ``render``'s (rgb, maps) of these rays, for the upstream g_rgb [N, 3] and g_maps [N, 2] (None: zeros),
    with respect to vol.sigma and vol.coef, ACCUMULATED into ``grad`` (grad_buffers).  The sums are integers: the accumulators hold the
    same bits whatever the ray order, the batch split or vol.block.  Misses and rays with an upstream value that is not finite add
    nothing.  The early end at t_stop is a constant of the gradient.  -> grad"""
    _dense_only(vol, "volume.render_backward")
    _on_device(vol.sigma, "volume.render_backward")
    dt = default_dt(vol) if dt is None else float(dt)
    ops.volume_render_backward(vol.sigma.detach(), vol.coef.detach(), vol.occ, vol.block, vol.lo.tolist(), vol.step.tolist(),
                               _on_device(origins, "volume.render_backward"), torch.as_tensor(dirs), tmin, tmax, dt, t_stop, background,
                               _on_device(g_rgb, "volume.render_backward"), None if g_maps is None else torch.as_tensor(g_maps),
                               grad.acc_sigma, grad.acc_coef)
    return grad


def gradients(grad, scale=1.0):
    """The accumulators read as fp32: (d_sigma [nx, ny, nz], d_coef [nx, ny, nz, ncoef, 3]) = fp32((double(acc) 2^-40) scale)."""
    f = lambda a: ((a.to(torch.float64) * 2.0 ** -_abi.VOLUME_GRAD_SHIFT) * float(scale)).to(torch.float32)
    return f(grad.acc_sigma), f(grad.acc_coef)


class _RenderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigma, coef, vol, origins, dirs, tmin, tmax, dt, t_stop, background):
        rgb, maps, steps = ops.volume_render(sigma.detach(), coef.detach(), vol.occ, vol.block, vol.lo.tolist(), vol.step.tolist(), origins, dirs,
                                             tmin, tmax, dt, t_stop, background)
        ctx.vol = vol._replace(sigma=sigma.detach(), coef=coef.detach())
        ctx.args = (origins, dirs, tmin, tmax, dt, t_stop, background)
        ctx.mark_non_differentiable(steps)
        return rgb, maps, steps

    @staticmethod
    def backward(ctx, g_rgb, g_maps, _g_steps):
        origins, dirs, tmin, tmax, dt, t_stop, background = ctx.args
        if g_rgb is None:
            g_rgb = torch.zeros(origins.reshape(-1, 3).shape[0], 3, device=ctx.vol.sigma.device)
        grad = render_backward(ctx.vol, grad_buffers(ctx.vol), origins, dirs, tmin, tmax, g_rgb, g_maps, dt=dt, t_stop=t_stop,
                               background=background)
        d_sigma, d_coef = gradients(grad)
        return (d_sigma if ctx.needs_input_grad[0] else None, d_coef if ctx.needs_input_grad[1] else None) + (None,) * 8


def render_train(vol, origins, dirs, tmin, tmax, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """``render`` under torch.autograd: the same (rgb, maps, steps), bit for bit, with rgb and maps carrying gradients to vol.sigma and
    vol.coef where those require them (render_backward into fresh grad_buffers, then gradients).  vol.occ must be blocks(vol.sigma,
    vol.block) of the CURRENT sigma, or a superset of it."""
    _dense_only(vol, "volume.render_train")
    _on_device(vol.sigma, "volume.render_train")
    dt = default_dt(vol) if dt is None else float(dt)
    return _RenderTrain.apply(vol.sigma, vol.coef, vol, _on_device(origins, "volume.render_train"), torch.as_tensor(dirs), tmin, tmax, dt,
                              float(t_stop), tuple(float(b) for b in background))


def member_mask(vol, index):
    """Rule VM: member[nx, ny, nz] uint8, 1 at the lattice points of ``index`` (an active list of ``vol``'s lattice), 0 elsewhere."""
    _on_device(vol.sigma, "volume.member_mask")
    return ops.volume_member_mask(_on_device(index, "volume.member_mask"), vol.sigma.shape)


def tv_backward(vol, grad, index, member, w_sigma, w_coef, eps=1e-9):
    """Rule VT: the gradient of w_sigma sum_p tau_sigma(p) + w_coef sum_p sum_words tau(p), p over the members, with respect to
    vol.sigma and vol.coef, ACCUMULATED into ``grad`` (grad_buffers) for the words of the points ``index`` (distinct; the level's list
    or a chunk of it -- ``member`` is member_mask of the whole list).  tau(p) = sqrt(sum_a d_a(p)^2 + eps) over the forward differences
    to members.  Points outside the mask receive nothing; the integers added to one word type sum to 0.  -> grad"""
    _dense_only(vol, "volume.tv_backward")
    _on_device(vol.sigma, "volume.tv_backward")
    ops.volume_tv_backward(vol.sigma.detach(), vol.coef.detach(), _on_device(index, "volume.tv_backward"), member, w_sigma, w_coef, eps,
                           grad.acc_sigma, grad.acc_coef)
    return grad


def upsampled_shape(shape):
    return tuple(2 * int(n) - 1 for n in shape)


def upsample(vol):
    """Rule VX: a new Volume on the lattice of 2 n - 1 points per axis over the same box (the step halved exactly), every value
    the trilinear mean of rule VL at f = 0.5 or the coarse value itself.  The block edge is kept; the occupancy is rebuilt by
    ``blocks``.  The input keeps its bits."""
    _dense_only(vol, "volume.upsample")
    _on_device(vol.sigma, "volume.upsample")
    sigma2, coef2 = ops.volume_upsample(vol.sigma.detach(), vol.coef.detach())
    step2 = (np.asarray(vol.step, np.float32) * np.float32(0.5)).astype(np.float32)
    return Volume(sigma2, coef2, blocks(sigma2, vol.block), np.asarray(vol.lo, np.float32).copy(), step2, vol.block, vol.degree)


def prune(vol, sigma_min):
    """Rule VP on copies: sigma not > sigma_min (finite, >= 0) becomes 0, and the coefficients of every point that is then not active
    (rule VA) become 0 -> a new Volume with its occupancy rebuilt.  sigma_min = 0 clears only stale coefficients.  The input keeps
    its bits."""
    _dense_only(vol, "volume.prune")
    _on_device(vol.sigma, "volume.prune")
    sigma, coef = ops.volume_prune(vol.sigma.detach().clone(), vol.coef.detach().clone(), sigma_min)
    return vol._replace(sigma=sigma, coef=coef, occ=blocks(sigma, vol.block))


_prune = prune  # finetune's keyword ``prune`` hides the function


class Finetuner:
    """Adam on a baked volume's sigma and coefficients against target pixels, the support frozen (rule VU): it works on its own copies
    (the input volume keeps its bits) and holds the active list of the volume as baked, the moments [n, 1 + 3 ncoef], the int64
    accumulators and the step count.  A sigma that reaches 0 stays 0, so the baked occupancy stays valid throughout.  The default rates
    are starting values from a CPU prototype on a hand-made volume, not a measurement on a scene.

    tv_sigma / tv_coef > 0 add a total-variation prior over the active list (rule VT): the loss becomes
    MSE + tv_sigma mean_p tau_sigma(p) + tv_coef mean_p sum_words tau(p), the means over the n members.  With both 0 no mask is
    allocated and no kernel is launched: the tuner is the plain one, bit for bit."""

    def __init__(self, vol, lr_sigma=0.1, lr_coef=0.01, betas=(0.9, 0.999), eps=1e-8, tv_sigma=0.0, tv_coef=0.0, tv_eps=1e-9):
        _dense_only(vol, "volume.Finetuner")
        _on_device(vol.sigma, "volume.Finetuner")
        _check_tv(tv_sigma, tv_coef, tv_eps)
        self.vol = vol._replace(sigma=vol.sigma.detach().clone(), coef=vol.coef.detach().clone())
        self.index = active(vol.sigma)
        words = 1 + 3 * int(vol.coef.shape[3])
        self.m = torch.zeros(int(self.index.shape[0]), words, device=vol.sigma.device)
        self.v = torch.zeros_like(self.m)
        self.grad = grad_buffers(self.vol)
        self.lr_sigma, self.lr_coef, self.betas, self.eps = float(lr_sigma), float(lr_coef), (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0
        self.tv_sigma, self.tv_coef, self.tv_eps = float(tv_sigma), float(tv_coef), float(tv_eps)
        self.member = member_mask(self.vol, self.index) if (self.tv_sigma > 0.0 or self.tv_coef > 0.0) else None

    def step(self, origins, dirs, tmin, tmax, target, background=(0.0, 0.0, 0.0), dt=None, t_stop=1e-3):
        """One update on the rays' mean squared colour error against target [N, 3]: forward, g_rgb = 2 (rgb - target) with
        grad_scale = 1 / (3 N), backward, the TV prior's gradient when it is on (w = tv / n * 3 N: rule VU multiplies the whole
        accumulator by grad_scale), rule VU -> the batch's MSE before the update, a device scalar (no host sync)."""
        dev = self.vol.sigma.device
        rgb, _, _ = render(self.vol, origins, dirs, tmin, tmax, dt=dt, t_stop=t_stop, background=background)
        diff = rgb - torch.as_tensor(target).to(dev, torch.float32).reshape(-1, 3)
        n = max(int(rgb.shape[0]), 1)
        render_backward(self.vol, self.grad, origins, dirs, tmin, tmax, 2.0 * diff, None, dt=dt, t_stop=t_stop, background=background)
        if self.member is not None and int(self.index.shape[0]) > 0:
            k = 3.0 * n / int(self.index.shape[0])
            tv_backward(self.vol, self.grad, self.index, self.member, self.tv_sigma * k, self.tv_coef * k, self.tv_eps)
        self.steps += 1
        ops.volume_adam_step(self.vol.sigma, self.vol.coef, self.index, self.grad.acc_sigma, self.grad.acc_coef, self.m, self.v,
                             1.0 / (3.0 * n), self.steps, self.lr_sigma, self.lr_coef, self.betas[0], self.betas[1], self.eps)
        return (diff * diff).mean() if rgb.numel() else torch.zeros((), device=dev)

    def volume(self):
        """The current state as a Volume, its occupancy rebuilt by ``blocks`` (the arrays are the tuner's own, not copies)."""
        return self.vol._replace(occ=blocks(self.vol.sigma, self.vol.block))

    def refined(self, prune=None):
        """The next level of a coarse-to-fine schedule: this tuner's volume, pruned (rule VP at ``prune``) unless that is None, refined
        (rule VX) -> a FRESH Finetuner on it with the same rates and TV weights: a new active list, zero moments, the step count at 0.
        This tuner's moments, accumulators and mask are released first; it takes no further step."""
        level = self.volume()
        self.m = self.v = self.grad = self.member = None
        if prune is not None:
            level = _prune(level, prune)
        return Finetuner(upsample(level), lr_sigma=self.lr_sigma, lr_coef=self.lr_coef, betas=self.betas, eps=self.eps,
                         tv_sigma=self.tv_sigma, tv_coef=self.tv_coef, tv_eps=self.tv_eps)


def _check_tv(tv_sigma, tv_coef, tv_eps):
    for name, w in (("tv_sigma", tv_sigma), ("tv_coef", tv_coef)):
        if not (np.isfinite(float(w)) and float(w) >= 0.0):
            raise ValueError(f"{name}={w!r}: a finite weight >= 0")
    if not (np.isfinite(float(tv_eps)) and float(tv_eps) > 0.0):
        raise ValueError(f"tv_eps={tv_eps!r}: finite and > 0")


def check_schedule(shape, iters, upsample_at=(), prune=None):
    """Validates a coarse-to-fine schedule for a lattice of ``shape`` (ValueError) -> (the sorted step counts as a tuple, the final
    lattice's shape): strictly increasing ints in (0, iters), every level's lattice below 2^31 points, prune None or finite and >= 0."""
    iters = int(iters)
    ups = []
    for u in upsample_at:
        if isinstance(u, bool) or int(u) != u:
            raise ValueError(f"upsample_at={tuple(upsample_at)!r}: step counts are ints")
        ups.append(int(u))
    for i, u in enumerate(ups):
        if not (0 < u < iters):
            raise ValueError(f"upsample_at={tuple(ups)!r}: every step count lies in (0, iters={iters})")
        if i and not ups[i - 1] < u:
            raise ValueError(f"upsample_at={tuple(ups)!r}: strictly increasing")
    if prune is not None and not (np.isfinite(float(prune)) and float(prune) >= 0.0):
        raise ValueError(f"prune={prune!r}: None, or a finite density >= 0")
    shape = tuple(int(n) for n in shape)
    for _ in ups:
        shape = upsampled_shape(shape)
        if shape[0] * shape[1] * shape[2] >= 2**31:
            raise ValueError(f"upsample_at={tuple(ups)!r}: the lattice {shape} of the last level must stay below 2^31 points")
    return tuple(ups), shape


def finetune(vol, rays, K_inv, iters, batch=4096, seed=None, background=(0.0, 0.0, 0.0), upsample_at=(), prune=None, **lrs):
    """``iters`` Finetuner steps on batches of ``batch`` pixels drawn (with replacement) from the data.DeviceRays ``rays``: the origin is
    the pose's translation, the direction ops.rays' unit d_wrd (as mesh.camera_rays forms it), the window the pose's near / far, the
    target the pixel's colour.  lrs: Finetuner's keywords (the rates and the TV weights).

    COARSE TO FINE.  ``upsample_at``: strictly increasing step counts in (0, iters); after that many steps the tuner's volume is pruned
    (``prune``: None, or rule VP's threshold) and refined (``upsample``), the old tuner's buffers are released and a FRESH Finetuner
    takes over (Finetuner.refined): a new active list, zero moments, the bias correction restarting at step 1, the same rates and TV weights; the march's
    default dt follows the halved step.  The whole schedule is validated before the first step (ValueError).
    -> (the fine-tuned Volume, the batch losses [iters] on the device, all levels concatenated)."""
    _dense_only(vol, "volume.finetune")
    dev = _on_device(vol.sigma, "volume.finetune").device
    ups, _ = check_schedule(vol.sigma.shape, iters, upsample_at, prune)
    _check_tv(lrs.get("tv_sigma", 0.0), lrs.get("tv_coef", 0.0), lrs.get("tv_eps", 1e-9))
    tuner, losses = _finetune_loop(Finetuner(vol, **lrs), rays, K_inv, iters, batch, seed, background, ups, prune, dev)
    return tuner.volume(), losses


def _finetune_loop(tuner, rays, K_inv, iters, batch, seed, background, ups, prune, dev):
    """finetune's steps for a tuner of either form -> (the last level's tuner, the batch losses [iters])"""
    gen = torch.Generator(device=dev)
    if seed is not None:
        gen.manual_seed(int(seed))
    losses = []
    for it in range(int(iters)):
        if it in ups:
            tuner = tuner.refined(prune)
        idx = torch.randint(int(rays.num_pix), (int(batch),), device=dev, generator=gen)
        row, col, pix, pb, _ = rays.gather(idx)
        _, d_wrd, _ = ops.rays(row, col, pb, torch.as_tensor(K_inv), 2)
        o = pb[:, :15].reshape(-1, 3, 5)[:, :, 3].contiguous()
        losses.append(tuner.step(o, d_wrd, pb[:, 15].contiguous(), pb[:, 16].contiguous(), pix, background=background))
    return tuner, (torch.stack(losses) if losses else torch.zeros(0, device=dev))


class CompactGrad(NamedTuple):
    acc_sigma: torch.Tensor   # [n] int64: sums of llrint(x 2^40), one per row
    acc_coef: torch.Tensor    # [n, 3 (degree + 1)^2] int64


def _compact_only(cvol, what):
    _no_vq(cvol, what)
    if not isinstance(cvol, CompactVolume):
        raise TypeError(f"{what} works on a volume.CompactVolume: volume.pack(vol) gives one; the dense volume.Volume has training "
                        "calls of its own (Finetuner, render_backward, tv_backward, finetune)")
    return cvol


def _fp32_rows(cvol, what):
    if cvol.coef.dtype != torch.float32:
        raise ValueError(f"{what}: a compact volume is trained on fp32 rows -- CompactFinetuner widens fp16 rows itself")


def convert(cvol, dtype):
    """cvol with its coefficient rows in ``dtype``: fp32 -> fp16 rounds with pack's own call on the rows seen as a small lattice
    ((n4 / 4, 2, 2), as NeRFModel.bake_volume converts them), fp16 -> fp32 widens (exact); the other arrays are shared.  Rounding
    holds a zeroed fp32 copy of the rows (the padded lattice) beside the input and the fp16 result until it returns: 12 ncoef bytes
    per row more, as the compact bake's own conversion."""
    half = _DTYPES[dtype]
    if (cvol.coef.dtype == torch.float16) == half:
        return cvol
    n, words = int(cvol.sigma.shape[0]), 3 * (cvol.degree + 1) ** 2
    if not half:
        return cvol._replace(coef=cvol.coef[:, :words].to(torch.float32).contiguous())
    n4 = max(8, (n + 3) // 4 * 4)
    lattice = torch.zeros(n4 // 4, 2, 2, (cvol.degree + 1) ** 2, 3, device=cvol.coef.device)
    lattice.reshape(n4, -1)[:n] = cvol.coef
    return cvol._replace(coef=ops.volume_compact_pack(None, lattice, None, True)[1][:n])


def row_points(cvol):
    """index[n] int32: the lattice point that holds row r (-1: none), from the slots that lie in [0, n).  For a packed volume this is
    rule VA's active list."""
    _compact_only(cvol, "volume.row_points")
    _on_device(cvol.slot, "volume.row_points")
    return _row_points(cvol)


def compact_grad_buffers(cvol):
    """Zeroed accumulators of rule VCG for ``cvol``, one int64 word per row word: 8 bytes per stored parameter."""
    _compact_only(cvol, "volume.compact_grad_buffers")
    dev = _on_device(cvol.slot, "volume.compact_grad_buffers").device
    n = int(cvol.sigma.shape[0])
    return CompactGrad(torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, 3 * (cvol.degree + 1) ** 2, dtype=torch.int64, device=dev))


def compact_render_backward(cvol, grad, origins, dirs, tmin, tmax, g_rgb, g_maps=None, dt=None, t_stop=1e-3, background=(0.0, 0.0, 0.0)):
    """Rule VCG: ``render_backward`` over a CompactVolume with fp32 rows, ACCUMULATED into ``grad`` (compact_grad_buffers): row r
    receives, bit for bit, what render_backward on unpack(cvol) adds at the row's lattice point; a corner without a row receives
    nothing.  The same bits whatever the ray order, the batch split or cvol.block.  -> grad"""
    _compact_only(cvol, "volume.compact_render_backward")
    _on_device(cvol.slot, "volume.compact_render_backward")
    _fp32_rows(cvol, "volume.compact_render_backward")
    dt = default_dt(cvol) if dt is None else float(dt)
    ops.volume_compact_render_backward(cvol.slot, cvol.sigma.detach(), cvol.coef.detach(), cvol.degree, cvol.occ, cvol.block, cvol.lo.tolist(),
                                       cvol.step.tolist(), _on_device(origins, "volume.compact_render_backward"), torch.as_tensor(dirs), tmin,
                                       tmax, dt, t_stop, background, _on_device(g_rgb, "volume.compact_render_backward"),
                                       None if g_maps is None else torch.as_tensor(g_maps), grad.acc_sigma, grad.acc_coef)
    return grad


def compact_tv_backward(cvol, grad, w_sigma, w_coef, eps=1e-9):
    """Rule VCT: ``tv_backward`` over a CompactVolume with fp32 rows, the members being the points with a row, ACCUMULATED into
    ``grad`` (compact_grad_buffers): bit for bit tv_backward on unpack(cvol) with member_mask(row_points(cvol)), gathered at the
    rows.  NOT enqueue-only: every call rebuilds the row -> point list from the slot lattice (row_points: passes over the whole
    lattice and one host sync).  A caller that repeats it uses CompactFinetuner, which keeps the list, or
    ops.volume_compact_tv_backward with row_points(cvol) cached.  -> grad"""
    _compact_only(cvol, "volume.compact_tv_backward")
    _on_device(cvol.slot, "volume.compact_tv_backward")
    _fp32_rows(cvol, "volume.compact_tv_backward")
    ops.volume_compact_tv_backward(cvol.slot, cvol.sigma.detach(), cvol.coef.detach(), cvol.degree, _row_points(cvol), w_sigma, w_coef, eps,
                                   grad.acc_sigma, grad.acc_coef)
    return grad


class CompactFinetuner:
    """``Finetuner`` on the compact form (rules VCG, VCU and VCT): Adam on the ROWS of a CompactVolume, the
    accumulators and the moments one per row -- 112 + 224 + 224 + 4 bytes per row at degree 2 beside the slot lattice, instead of a
    dense working copy, dense int64 accumulators and a member mask.  It works on its own copies of the rows (fp16 rows are widened,
    exactly; training is in fp32) and shares the slot lattice, which never changes.  Every step equals Finetuner(unpack(cvol))'s bit
    for bit: the same losses, and the same values at the rows."""

    def __init__(self, cvol, lr_sigma=0.1, lr_coef=0.01, betas=(0.9, 0.999), eps=1e-8, tv_sigma=0.0, tv_coef=0.0, tv_eps=1e-9):
        _compact_only(cvol, "volume.CompactFinetuner")
        _on_device(cvol.slot, "volume.CompactFinetuner")
        _check_tv(tv_sigma, tv_coef, tv_eps)
        words = 3 * (cvol.degree + 1) ** 2
        self.cvol = cvol._replace(sigma=cvol.sigma.detach().clone(), coef=cvol.coef.detach()[:, :words].to(torch.float32, copy=True).contiguous())
        self.point = _row_points(cvol)
        n = int(cvol.sigma.shape[0])
        self.m = torch.zeros(n, 1 + words, device=cvol.slot.device)
        self.v = torch.zeros_like(self.m)
        self.grad = compact_grad_buffers(self.cvol)
        self.lr_sigma, self.lr_coef, self.betas, self.eps = float(lr_sigma), float(lr_coef), (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0
        self.tv_sigma, self.tv_coef, self.tv_eps = float(tv_sigma), float(tv_coef), float(tv_eps)

    def step(self, origins, dirs, tmin, tmax, target, background=(0.0, 0.0, 0.0), dt=None, t_stop=1e-3):
        """Finetuner.step on the rows: the same scaling (grad_scale = 1 / (3 N), the TV weights times 3 N / n) -> the batch's MSE
        before the update, a device scalar (no host sync)."""
        c, dev = self.cvol, self.cvol.slot.device
        rgb, _, _ = render(c, origins, dirs, tmin, tmax, dt=dt, t_stop=t_stop, background=background)
        diff = rgb - torch.as_tensor(target).to(dev, torch.float32).reshape(-1, 3)
        n = max(int(rgb.shape[0]), 1)
        rows = int(c.sigma.shape[0])
        compact_render_backward(c, self.grad, origins, dirs, tmin, tmax, 2.0 * diff, None, dt=dt, t_stop=t_stop, background=background)
        if (self.tv_sigma > 0.0 or self.tv_coef > 0.0) and rows > 0:
            k = 3.0 * n / rows
            ops.volume_compact_tv_backward(c.slot, c.sigma, c.coef, c.degree, self.point, self.tv_sigma * k, self.tv_coef * k, self.tv_eps,
                                           self.grad.acc_sigma, self.grad.acc_coef)
        self.steps += 1
        ops.volume_compact_adam_step(c.sigma, c.coef, c.degree, self.grad.acc_sigma, self.grad.acc_coef, self.m, self.v, 1.0 / (3.0 * n),
                                     self.steps, self.lr_sigma, self.lr_coef, self.betas[0], self.betas[1], self.eps)
        return (diff * diff).mean() if rgb.numel() else torch.zeros((), device=dev)

    def volume(self, dtype="fp32"):
        """The current state REPACKED as a CompactVolume with ``dtype`` coefficients: a temporary dense sigma (4 bytes per lattice
        point) from the rows -> active -> new slots -> the kept rows gathered -> blocks.  Rows that rule VA no longer keeps -- a sigma
        that reached 0 took its neighbourhood's last positive value with it -- are dropped, so the result equals
        pack(Finetuner(unpack(cvol)) ... .volume(), dtype) bit for bit in slot, sigma, coef and occ."""
        if dtype not in _DTYPES:
            raise ValueError(f"dtype={dtype!r}: 'fp32' or 'fp16'")
        c = self.cvol
        n = int(c.sigma.shape[0])
        sigma, _ = ops.volume_compact_unpack(c.sigma, None, self.point, c.shape, c.degree)
        index = active(sigma)
        old = c.slot.reshape(-1)[index.long()].long()
        kept = (old >= 0) & (old < n)  # a point of the new list without a row holds +0, as it does in unpack(cvol)
        old = old.clamp(0, max(n - 1, 0))  # (without rows sigma is all +0 and the new list is empty)
        zero = torch.zeros((), device=sigma.device)
        sigma_rows, coef_rows = torch.where(kept, c.sigma[old], zero), torch.where(kept[:, None], c.coef[old], zero)
        out = c._replace(slot=ops.volume_compact_slots(index, c.shape), sigma=sigma_rows, coef=coef_rows, occ=blocks(sigma, c.block))
        return convert(out, dtype)

    def refined(self, prune=None):
        """Finetuner.refined through a TRANSIENT DENSE LEVEL: this tuner's volume unpacked, pruned (rule VP at ``prune``) unless that is
        None, refined (rule VX), packed -> a FRESH CompactFinetuner on it with the same rates and TV weights.  The dense coarse and fine
        levels live until the pack: compact upsample / prune kernels do not exist.  This tuner's buffers are released first."""
        level = unpack(self.volume())
        self.m = self.v = self.grad = self.point = self.cvol = None
        if prune is not None:
            level = _prune(level, prune)
        return CompactFinetuner(pack(upsample(level)), lr_sigma=self.lr_sigma, lr_coef=self.lr_coef, betas=self.betas, eps=self.eps,
                                tv_sigma=self.tv_sigma, tv_coef=self.tv_coef, tv_eps=self.tv_eps)


def finetune_compact(cvol, rays, K_inv, iters, batch=4096, seed=None, background=(0.0, 0.0, 0.0), upsample_at=(), prune=None, **lrs):
    """``finetune`` with a CompactFinetuner: the same validation, the same batches for the same seed, the same schedule (each
    refinement through CompactFinetuner.refined's transient dense level) -> (the fine-tuned CompactVolume with fp32 rows, the batch
    losses [iters] on the device).  Bit for bit pack(finetune(unpack(cvol), ...)[0]) and its losses when ``prune`` is given."""
    _compact_only(cvol, "volume.finetune_compact")
    dev = _on_device(cvol.slot, "volume.finetune_compact").device
    ups, _ = check_schedule(cvol.shape, iters, upsample_at, prune)
    _check_tv(lrs.get("tv_sigma", 0.0), lrs.get("tv_coef", 0.0), lrs.get("tv_eps", 1e-9))
    tuner, losses = _finetune_loop(CompactFinetuner(cvol, **lrs), rays, K_inv, iters, batch, seed, background, ups, prune, dev)
    return tuner.volume(), losses


def save(path, vol):
    """The volume as a plain ``.npz`` (numpy.savez: sigma, coef, occ, lo, step, block, degree).  A CompactVolume is written with the
    keys slot, sigma_rows, coef_rows (fp32 or fp16), occ, lo, step, block, degree: the key ``slot`` tells the forms apart.  A VQVolume
    is written with the keys mask (numpy.packbits of the lattice: 1 where a point has a row), sigma_rows, cls, code, kept, codebook,
    lo, step, block, degree, shape: the key ``codebook`` tells it from the other two."""
    if isinstance(vol, VQVolume):
        return _save_vq(path, vol)
    if isinstance(vol, CompactVolume):
        with open(path, "wb") as f:
            np.savez(f, slot=vol.slot.cpu().numpy(), sigma_rows=vol.sigma.detach().cpu().numpy(), coef_rows=vol.coef.detach().cpu().numpy(),
                     occ=vol.occ.cpu().numpy(), lo=np.asarray(vol.lo, np.float32), step=np.asarray(vol.step, np.float32),
                     block=np.int64(vol.block), degree=np.int64(vol.degree))
        return
    with open(path, "wb") as f:
        np.savez(f, sigma=vol.sigma.detach().cpu().numpy(), coef=vol.coef.detach().cpu().numpy(), occ=vol.occ.detach().cpu().numpy(),
                 lo=np.asarray(vol.lo, np.float32), step=np.asarray(vol.step, np.float32), block=np.int64(vol.block),
                 degree=np.int64(vol.degree))


def load(path, device="cuda"):
    """save()'s file -> the form it holds, a Volume, (a file with the key ``slot``) a CompactVolume or (the key ``codebook``) a
    VQVolume, on ``device`` with the saved bits."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("volume.load puts the volume on a ROCm device (MI355X): there is no CPU path")
    with np.load(path) as z:
        t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(dev)
        if "codebook" in z.files:
            return _load_vq(z, dev)
        if "slot" in z.files:
            slot = t("slot")
            return CompactVolume(slot, t("sigma_rows"), t("coef_rows"), t("occ"), z["lo"].astype(np.float32).reshape(3),
                                 z["step"].astype(np.float32).reshape(3), int(z["block"]), int(z["degree"]), tuple(int(n) for n in slot.shape))
        return Volume(t("sigma"), t("coef"), t("occ"), z["lo"].astype(np.float32).reshape(3), z["step"].astype(np.float32).reshape(3),
                      int(z["block"]), int(z["degree"]))


# ---- vector-quantised volumes (rules VI, VQ-A, VQ-U and VQ-D of include/nerf_hip.h) ----

VQ_MAX_CODES = ops.VQ_MAX_CODES
VQ_MAX_WORD = 1024.0  # rule VQ-U's bound on a coded word: a row with a larger or non-finite word is kept verbatim


class VQVolume(NamedTuple):
    point: torch.Tensor     # [n] int32: the lattice point of each row, ascending (rule VA's list of the volume it came from)
    sigma: torch.Tensor     # [n] fp32: the rows' sigma; a pruned row holds +0
    cls: torch.Tensor       # [n] uint8: 0 pruned, 1 coded, 2 kept
    code: torch.Tensor      # [n_coded] uint16: the coded rows' codes, in row order
    kept: torch.Tensor      # [n_kept, S] fp16: the kept rows verbatim (rule VC's fp16 rows), in row order
    codebook: torch.Tensor  # [K', S] fp16
    lo: np.ndarray          # [3] fp32
    step: np.ndarray        # [3] fp32
    block: int
    degree: int
    shape: tuple            # (nx, ny, nz)


def _vq_cvol(cvol, what):
    if not isinstance(cvol, CompactVolume):
        raise TypeError(f"{what} works on a volume.CompactVolume (volume.pack(vol) gives one; volume.dequantize(vq) turns a VQVolume "
                        f"back into one), not on {type(cvol).__name__}")
    _on_device(cvol.slot, what)
    return cvol


def importance(cvol, origins, dirs, tmin, tmax, acc=None, dt=None, t_stop=1e-3):
    """Rule VI: the rendering weight every ROW of ``cvol`` receives from these rays -- render's march (the same samples, the same
    w = T alpha, the same end at t_stop), each contributing sample's w split over the cell's corners by the trilinear terms and added
    to the corners' rows in int64 fixed point (units of 2^-40, as the gradient accumulators).  Either row dtype: no coefficient is
    read.  ``acc`` [n] int64 is ADDED to (a zeroed one is made when None), so batches and views accumulate; the sums hold the same
    bits whatever the ray order, the batch split or cvol.block.  -> (acc, steps [N, 2] = render's own steps)"""
    _vq_cvol(cvol, "volume.importance")
    n = int(cvol.sigma.shape[0])
    if acc is None:
        acc = torch.zeros(n, dtype=torch.int64, device=cvol.slot.device)
    dt = default_dt(cvol) if dt is None else float(dt)
    steps = ops.volume_compact_importance(cvol.slot, cvol.sigma.detach(), cvol.occ, cvol.block, cvol.lo.tolist(), cvol.step.tolist(),
                                          _on_device(origins, "volume.importance"), torch.as_tensor(dirs), tmin, tmax, dt, t_stop, acc)
    return acc, steps


def importance_views(cvol, poses_bound17, K_inv, H, W, acc=None, views_per_call=None, dt=None, t_stop=1e-3):
    """``importance`` over the cameras poses_bound17 [n, 17] along render_views' own rays (mesh.camera_rays; each camera's window its
    near / far), ``views_per_call`` cameras per call (None: all at once) -> (acc, steps [n, H, W, 2])."""
    from . import mesh

    dev = _vq_cvol(cvol, "volume.importance_views").slot.device
    pb = torch.as_tensor(poses_bound17).to(dev, torch.float32).reshape(-1, 17)
    n, H, W = int(pb.shape[0]), int(H), int(W)
    per = n if views_per_call is None else int(views_per_call)
    if n and per < 1:
        raise ValueError(f"views_per_call={views_per_call!r}: an int >= 1")
    if acc is None:
        acc = torch.zeros(int(cvol.sigma.shape[0]), dtype=torch.int64, device=dev)
    steps = []
    for v0 in range(0, n, max(per, 1)):
        part = pb[v0:v0 + per]
        o, d = mesh.camera_rays(part, K_inv, H, W, device=dev)
        near, far = part[:, 15].repeat_interleave(H * W), part[:, 16].repeat_interleave(H * W)
        steps.append(importance(cvol, o, d, near, far, acc=acc, dt=dt, t_stop=t_stop)[1])
    steps = torch.cat(steps) if steps else torch.zeros(0, 2, dtype=torch.int32, device=dev)
    return acc, steps.view(n, H, W, 2)


def _share(share, what):
    from fractions import Fraction

    f = Fraction(share)
    if not 0 <= f <= 1:
        raise ValueError(f"{what}={share!r}: a share lies in [0, 1]")
    return f


def vq_classes(imp, prune_share=None, keep_share=0.0, rows=None):
    """The class of every row from its importance imp [n] (int64, >= 0) -> cls [n] uint8: 0 pruned, 1 coded, 2 kept.  EXACT: the rows
    are ordered by (imp ascending, row ascending) -- a stable sort --, the running sums are int64 and the thresholds integers,
    floor(Fraction(share) * total):
      * pruned: the rows from the bottom of the order whose running sum is <= floor(prune_share * total); prune_share = None prunes
        nothing, not even a row of importance 0 (prune_share = 0 prunes exactly those at the bottom);
      * kept: the rows from the top of the order whose running sum FROM THE TOP is <= floor(keep_share * total);
      * a row that is both is pruned; every other row is coded;
      * with ``rows`` [n, W] (fp32 or fp16): a row with a non-finite word or one of magnitude above 1024 is kept whatever its
        importance -- rule VQ-U's overflow bound needs the coded words within 2^10.
    One host read (the total).  The one call of this family that also takes CPU tensors: there is no kernel in it."""
    imp = torch.as_tensor(imp)  # exact integer plumbing: it runs wherever imp lives
    if imp.dtype != torch.int64 or imp.dim() != 1:
        raise ValueError(f"imp {tuple(imp.shape)} {imp.dtype}: int64 [n]")
    n, dev = int(imp.shape[0]), imp.device
    prune = None if prune_share is None else _share(prune_share, "prune_share")
    keep = _share(keep_share, "keep_share")
    cls = torch.ones(n, dtype=torch.uint8, device=dev)
    if n:
        if int(imp.min()) < 0:
            raise ValueError("imp: an importance is a sum of weights, >= 0")
        srt, order = torch.sort(imp, stable=True)
        cs = torch.cumsum(srt, 0)
        total = int(cs[-1])
        from_top = (total - cs) + srt
        kept = from_top <= int(keep * total)
        cls[order[kept]] = 2
        if prune is not None:
            cls[order[cs <= int(prune * total)]] = 0
    if rows is not None:
        if tuple(rows.shape[:1]) != (n,) or rows.device != dev:
            raise ValueError(f"rows {tuple(rows.shape)}: one per importance ({n}) on its device")
        r32 = rows.to(torch.float32)
        cls[~(torch.isfinite(r32) & (r32.abs() <= VQ_MAX_WORD)).all(dim=1)] = 2
    return cls


def _check_k(K, iters=0):
    if int(K) != K or not 1 <= int(K) <= VQ_MAX_CODES:
        raise ValueError(f"K={K!r}: a codebook has 1 .. {VQ_MAX_CODES} codes (a code is a uint16)")
    if int(iters) != iters or int(iters) < 0:
        raise ValueError(f"iters={iters!r}: an int >= 0")
    return int(K), int(iters)


def kmeans(rows, weight, K, iters):
    """Weighted k-means over the fp32 rows [m, W] (rules VQ-A and VQ-U) -> (codebook [K', W] fp32, assign [m] int32), K' = min(K, m).
    INIT: codebook[j] is the row at position (j m) // K' of the order (weight descending, row ascending) -- with K' = m every row is
    its own code.  ONE ITERATION: assign, zero the sums, accumulate, update; after ``iters`` of them one more assign gives the codes.
    weight [m] int64 >= 0 or None (every row counts 1).  Every step is exact or a fixed order of fp32 roundings, the sums are int64:
    the result has one value, whatever the order the device works in.  One host read (the largest weight)."""
    rows = _on_device(rows, "volume.kmeans")
    K, iters = _check_k(K, iters)
    m, dev = int(rows.shape[0]), rows.device
    if weight is not None:
        if weight.dtype != torch.int64 or tuple(weight.shape) != (m,) or weight.device != dev:
            raise ValueError(f"weight: int64 [{m}] on the rows' device")
        if m and int(weight.min()) < 0:
            raise ValueError("weight: an importance is a sum of weights, >= 0")
    if m == 0:
        return rows.new_zeros((0,) + tuple(rows.shape[1:])), torch.zeros(0, dtype=torch.int32, device=dev)
    Kp = min(K, m)
    order = torch.arange(m, device=dev) if weight is None else torch.sort(weight, descending=True, stable=True)[1]
    codebook = rows[order[(torch.arange(Kp, device=dev) * m) // Kp]].contiguous().clone()
    imax = 0 if weight is None else int(weight.max())
    weight = None if weight is None else weight.contiguous()
    sums = counts = None
    for _ in range(iters):
        assign = ops.volume_vq_assign(rows, codebook)
        if sums is not None:
            sums.zero_(), counts.zero_()
        sums, counts = ops.volume_vq_accumulate(rows, weight, imax, assign, Kp, sums, counts)
        ops.volume_vq_update(codebook, sums, counts)
    return codebook, ops.volume_vq_assign(rows, codebook)


def _rows_to_half(rows32, degree):
    """fp32 rows [k, 3 ncoef] -> rule VC's fp16 rows [k, S] (+0 pads), rounded by pack's own call as ``convert`` rounds"""
    k = int(rows32.shape[0])
    k4 = max(8, (k + 3) // 4 * 4)
    lattice = torch.zeros(k4 // 4, 2, 2, (degree + 1) ** 2, 3, device=rows32.device)
    lattice.reshape(k4, -1)[:k] = rows32
    return ops.volume_compact_pack(None, lattice, None, True)[1][:k].contiguous()


def quantize(cvol, imp, K=4096, iters=10, prune_share=None, keep_share=0.0):
    """``cvol`` as a VQVolume (VQRF's three steps): vq_classes(imp, prune_share, keep_share, rows) sorts the rows into pruned, coded and
    kept; the coded rows (fp16 rows widened first, exactly) are clustered by kmeans(.., weight = their importance, K, iters); the
    codebook and the kept rows are rounded to fp16 ONCE, with convert's rule.  A pruned row keeps its place in the list with sigma +0
    -- sigma stays fp32 and no other sigma moves, so the support and rule VA's list are those of ``cvol``.  The rows of ``cvol`` must
    be in the order of their lattice points (pack and the compact bake make them so)."""
    _vq_cvol(cvol, "volume.quantize")
    K, iters = _check_k(K, iters)
    n, words, dev = int(cvol.sigma.shape[0]), 3 * (cvol.degree + 1) ** 2, cvol.slot.device
    imp = _on_device(imp, "volume.quantize")
    if imp.dtype != torch.int64 or tuple(imp.shape) != (n,):
        raise ValueError(f"imp {tuple(imp.shape)} {imp.dtype}: int64, one per row ({n})")
    point = _row_points(cvol)
    if n and (int(point[0]) < 0 or (n > 1 and not bool((point[1:] > point[:-1]).all()))):
        raise ValueError("volume.quantize: the rows are not in the order of their lattice points (or a row has no point)")
    rows32 = cvol.coef.detach()[:, :words].to(torch.float32).contiguous()
    cls = vq_classes(imp, prune_share, keep_share, rows=rows32)
    coded = cls == 1
    codebook, assign = kmeans(rows32[coded].contiguous(), imp[coded].contiguous(), K, iters)
    zero = torch.zeros((), device=dev)
    return VQVolume(point, torch.where(cls == 0, zero, cvol.sigma.detach()), cls, assign.to(torch.uint16),
                    _rows_to_half(rows32[cls == 2], cvol.degree), _rows_to_half(codebook, cvol.degree),
                    np.asarray(cvol.lo, np.float32), np.asarray(cvol.step, np.float32), cvol.block, cvol.degree, tuple(cvol.shape))


def dequantize(vq):
    """Rule VQ-D: the VQVolume as a CompactVolume with fp16 rows -- the slots from ``point`` (volume_compact_slots), every row from
    its class (a coded row copies its code's words, a kept row its own, a pruned row is +0 with sigma +0), occ rebuilt from the
    decoded sigma as with_block does.  The device-side form is rule VC's again: the quantised form makes the FILE small, not the
    memory the marcher reads."""
    if not isinstance(vq, VQVolume):
        raise TypeError("volume.dequantize takes a VQVolume")
    _on_device(vq.point, "volume.dequantize")
    cls = vq.cls
    coded, kept = cls == 1, cls == 2
    rank = torch.where(coded, torch.cumsum(coded, 0) - 1, torch.where(kept, torch.cumsum(kept, 0) - 1, 0)).to(torch.int32)
    rows = ops.volume_vq_decode(cls.contiguous(), rank.contiguous(), vq.code, vq.kept, vq.codebook, vq.degree)
    slot = ops.volume_compact_slots(vq.point, vq.shape)
    sigma, _ = ops.volume_compact_unpack(vq.sigma, None, vq.point, vq.shape, vq.degree)
    return CompactVolume(slot, vq.sigma, rows, blocks(sigma, vq.block), np.asarray(vq.lo, np.float32), np.asarray(vq.step, np.float32),
                         vq.block, vq.degree, tuple(vq.shape))


# ---- fine-tuning the quantised form (rules VQ-X, VQ-G and VQ-V of include/nerf_hip.h) ----

VQ_MAX_RAYS = ops.VQ_MAX_RAYS  # rule VQ-G's overflow precondition: the rays of one update


def _vq_rank(cls):
    """rank [n] int32: a row's rank among the rows of its class, in row order (0 for a pruned row), as dequantize forms it"""
    coded, kept = cls == 1, cls == 2
    return torch.where(coded, torch.cumsum(coded, 0) - 1, torch.where(kept, torch.cumsum(kept, 0) - 1, 0)).to(torch.int32).contiguous()


def vq_members(cls, code, K):
    """The coded rows GROUPED BY CODE, as rule VQ-G reads them -> (offset [K + 1] int32, member [n_coded] int32): a stable sort of the
    codes, so the members of a code are in row order; offset is the exclusive prefix sum of the codes' counts.  A code >= K sorts
    past offset[K] and belongs to no group.  Exact integer plumbing, as vq_classes: it runs wherever cls lives."""
    rows = torch.nonzero(cls == 1).reshape(-1)
    c = code.to(torch.int64)
    if tuple(c.shape) != tuple(rows.shape):
        raise ValueError(f"code {tuple(code.shape)}: one per coded row ({int(rows.shape[0])})")
    order = torch.sort(c, stable=True)[1]
    counts = torch.bincount(c, minlength=int(K))[:int(K)]
    offset = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)
    return offset.contiguous(), rows[order].to(torch.int32).contiguous()


class VQFinetuner:
    """VQRF's fourth step (rules VQ-X, VQ-G and VQ-V): Adam on the CODEBOOK, the KEPT ROWS and SIGMA of a
    VQVolume against rays, the classes and the codes frozen.  It holds fp32 masters widened from the fp16 codebook and kept rows
    (exact), a working CompactVolume with fp32 rows expanded from them (the slots from ``point``, occ from sigma, as dequantize builds
    them) that the compact march and its gradient read, the per-row accumulators, one int64 accumulator row per code, the member lists
    (built once: the codes are frozen) and the moments -- per coded row 8 bytes of moments (its sigma) where CompactFinetuner holds
    8 (1 + W).  With every code holding one row, or every row kept, each step equals CompactFinetuner(dequantize(vq))'s bit for bit.
    No TV prior: VQRF uses none here."""

    def __init__(self, vq, lr_sigma=0.1, lr_coef=0.01, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(vq, VQVolume):
            raise TypeError("volume.VQFinetuner takes a VQVolume (volume.quantize gives one; CompactFinetuner trains a CompactVolume)")
        dev = _on_device(vq.point, "volume.VQFinetuner").device
        words = 3 * (vq.degree + 1) ** 2
        self.vq = vq
        self.cls, self.code, self.rank = vq.cls.contiguous(), vq.code.contiguous(), _vq_rank(vq.cls)
        self.kept32 = vq.kept[:, :words].to(torch.float32).contiguous()
        self.codebook32 = vq.codebook[:, :words].to(torch.float32).contiguous()
        n, n_kept, K = int(vq.sigma.shape[0]), int(self.kept32.shape[0]), int(self.codebook32.shape[0])
        sigma_rows = vq.sigma.detach().clone()
        rows = ops.volume_vq_expand(self.cls, self.rank, self.code, self.kept32, self.codebook32, vq.degree)
        sigma, _ = ops.volume_compact_unpack(sigma_rows, None, vq.point, vq.shape, vq.degree)
        self.cvol = CompactVolume(ops.volume_compact_slots(vq.point, vq.shape), sigma_rows, rows, blocks(sigma, vq.block),
                                  np.asarray(vq.lo, np.float32), np.asarray(vq.step, np.float32), vq.block, vq.degree, tuple(vq.shape))
        self.kept_row = torch.nonzero(self.cls == 2).reshape(-1).to(torch.int32).contiguous()
        self.offset, self.member = vq_members(self.cls, self.code, K)
        self.grad = compact_grad_buffers(self.cvol)
        self.acc_code = torch.zeros(K, words, dtype=torch.int64, device=dev)
        self.m = torch.zeros(n + (n_kept + K) * words, device=dev)
        self.v = torch.zeros_like(self.m)
        self.lr_sigma, self.lr_coef, self.betas, self.eps = float(lr_sigma), float(lr_coef), (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0

    def step(self, origins, dirs, tmin, tmax, target, background=(0.0, 0.0, 0.0), dt=None, t_stop=1e-3):
        """render the working rows -> the gradient of the batch's MSE into the rows' accumulators (rule VCG with 2 diff) -> the coded
        rows' words summed per code (VQ-G) -> one Adam launch over sigma, the kept rows and the codebook with grad_scale = 1 / (3 N)
        (VQ-V) -> the working rows rebuilt from the masters (VQ-X).  At most 2^20 rays (rule VQ-G's overflow precondition: ValueError);
        pixels and background are colours in [0, 1].  -> the batch's MSE before the update, a device scalar (no host sync)."""
        c, dev = self.cvol, self.cvol.slot.device
        if int(torch.as_tensor(origins).numel()) // 3 > VQ_MAX_RAYS:
            raise ValueError(f"volume.VQFinetuner.step: {int(torch.as_tensor(origins).numel()) // 3} rays -- one update takes at most 2^20 "
                             "(the int64 sums of a code's gradient are proved not to overflow up to there)")
        rgb, _, _ = render(c, origins, dirs, tmin, tmax, dt=dt, t_stop=t_stop, background=background)
        diff = rgb - torch.as_tensor(target).to(dev, torch.float32).reshape(-1, 3)
        n = max(int(rgb.shape[0]), 1)
        compact_render_backward(c, self.grad, origins, dirs, tmin, tmax, 2.0 * diff, None, dt=dt, t_stop=t_stop, background=background)
        ops.volume_vq_grad_reduce(self.grad.acc_coef, self.offset, self.member, self.acc_code)
        self.steps += 1
        ops.volume_vq_adam_step(c.sigma, self.kept32, self.kept_row, self.codebook32, c.degree, self.grad.acc_sigma, self.grad.acc_coef,
                                self.acc_code, self.m, self.v, 1.0 / (3.0 * n), self.steps, self.lr_sigma, self.lr_coef, self.betas[0],
                                self.betas[1], self.eps)
        ops.volume_vq_expand(self.cls, self.rank, self.code, self.kept32, self.codebook32, c.degree, out=c.coef, acc_coef_rows=self.grad.acc_coef)
        return (diff * diff).mean() if rgb.numel() else torch.zeros((), device=dev)

    def volume(self):
        """The current state as a VQVolume: the same point, cls and code, the current sigma (a copy), the codebook and the kept rows
        rounded to fp16 ONCE with quantize's rule.  A row whose sigma reached 0 keeps its class; the file format does not change."""
        vq = self.vq
        return vq._replace(sigma=self.cvol.sigma.detach().clone(), kept=_rows_to_half(self.kept32, vq.degree),
                           codebook=_rows_to_half(self.codebook32, vq.degree))


def finetune_vq(vq, rays, K_inv, iters, batch=4096, seed=None, background=(0.0, 0.0, 0.0), **lrs):
    """``finetune_compact`` with a VQFinetuner: the same batches for the same seed (finetune's own loop), no schedule -- a VQ volume is
    not refined -- -> (the fine-tuned VQVolume, the batch losses [iters] on the device).  lrs: VQFinetuner's keywords."""
    if not isinstance(vq, VQVolume):
        raise TypeError("volume.finetune_vq takes a VQVolume (volume.quantize gives one)")
    dev = _on_device(vq.point, "volume.finetune_vq").device
    if int(iters) != iters or int(iters) < 0:
        raise ValueError(f"iters={iters!r}: a number of steps >= 0")
    if int(batch) > VQ_MAX_RAYS:
        raise ValueError(f"batch={batch!r}: one update takes at most 2^20 rays")
    tuner, losses = _finetune_loop(VQFinetuner(vq, **lrs), rays, K_inv, iters, batch, seed, background, (), None, dev)
    return tuner.volume(), losses


def _save_vq(path, vq):
    """point is stored as a numpy.packbits mask of the lattice (1 bit per lattice point instead of 4 bytes per row or per point)"""
    npts = int(np.prod(vq.shape))
    mask = np.zeros(npts, bool)
    mask[vq.point.cpu().numpy().astype(np.int64)] = True
    with open(path, "wb") as f:
        np.savez(f, mask=np.packbits(mask), sigma_rows=vq.sigma.detach().cpu().numpy(), cls=vq.cls.cpu().numpy(), code=vq.code.cpu().numpy(),
                 kept=vq.kept.cpu().numpy(), codebook=vq.codebook.cpu().numpy(), lo=np.asarray(vq.lo, np.float32),
                 step=np.asarray(vq.step, np.float32), block=np.int64(vq.block), degree=np.int64(vq.degree),
                 shape=np.asarray(vq.shape, np.int64))


def _load_vq(z, dev):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(dev)
    shape = tuple(int(x) for x in z["shape"])
    mask = np.unpackbits(z["mask"], count=int(np.prod(shape))).astype(bool)
    point = torch.from_numpy(np.flatnonzero(mask).astype(np.int32)).to(dev)
    return VQVolume(point, t("sigma_rows"), t("cls"), t("code"), t("kept"), t("codebook"), z["lo"].astype(np.float32).reshape(3),
                    z["step"].astype(np.float32).reshape(3), int(z["block"]), int(z["degree"]), shape)
