"""Host-side mirror of the reference's ``nerf`` module surface for the volume-rendering hot path.

Same names, constructor arguments, call signatures and ``state_dict`` keys as the reference
(``/root/reference/nerf.py``): ``NeRFModel(num_coarse, num_fine, batch_ray)`` (nerf.py:170),
``model(row, column, poses_bound, K_inv) -> (C_coarse, C_fine)`` (nerf.py:333-348),
``model.ray_loss`` (nerf.py:325-331), ``model.network.parameters()`` for Adam (nerf.py:425).
The arithmetic happens in libnerf_hip.so (hand-written gfx950 kernels) through a
``torch.autograd.Function``; PyTorch only owns device memory, the stream and autograd plumbing.
There is NO fallback: calling a model that does not live on a ROCm device raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch
import torch.nn as nn

from . import _abi

# module-global device like the reference (nerf.py:40, :387); the model follows its parameters' device.
device = None

LAST_DELTA = 0.0001  # nerf.py:286
MIN_CALL_RAYS = 2     # include/nerf_hip.h: 2 <= B (the reference crashes on B = 1, nerf.py:208)


class Activation(nn.Module):
    """nerf.py:69-74 (abs); kept so pickled/introspected module trees look the same."""

    def forward(self, x):
        return torch.abs(x)


class Network(nn.Module):
    """Parameter container with the reference's module tree (nerf.py:76-99) so that ``state_dict``
    keys, shapes and ``parameters()`` order are identical.  The forward pass is the fused HIP kernel
    (csrc/field_fwd.hip); this module cannot be called on its own."""

    def __init__(self, point_dim=60, dir_dim=24, depth=8, width=256, batch_size=8, layers_skip=[4]):
        super().__init__()
        if (point_dim, dir_dim, depth, width, list(layers_skip)) != (60, 24, 8, 256, [4]):
            raise ValueError("libnerf_hip.so is built for the reference's architecture: 60/24 inputs, 8x256, skip at 4")
        self.depth, self.width, self.batch_size, self.layers_skip = depth, width, batch_size, layers_skip
        self.point_layer = nn.ModuleList([nn.Sequential(nn.Linear(point_dim, width), nn.ReLU(True))])
        for i in range(1, depth):
            fan_in = width + point_dim if i in layers_skip else width
            self.point_layer.append(nn.Sequential(nn.Linear(fan_in, width), nn.ReLU(True)))
        self.sigma_layer = nn.Sequential(nn.Linear(width, 1), Activation())
        self.point_info = nn.Linear(width, width)
        self.dir_info = nn.Sequential(nn.Linear(width + dir_dim, width // 2), nn.ReLU(True))
        self.color_layer = nn.Sequential(nn.Linear(width // 2, 3), nn.Sigmoid())

    def forward(self, *args, **kwargs):
        raise RuntimeError("Network is evaluated inside libnerf_hip.so (NeRFModel.forward); it has no eager path")


class Encoder(nn.Module):
    """nerf.py:126-167: no parameters; the encoding is fused into the field kernel."""

    def __init__(self, L_point=10, L_dir=4, batch_size=8):
        super().__init__()
        if (L_point, L_dir) != (10, 4):
            raise ValueError("libnerf_hip.so is built for L_point=10, L_dir=4")
        self.L_point, self.L_dir, self.batch_size = L_point, L_dir, batch_size

    def forward(self, *args, **kwargs):
        raise RuntimeError("Encoder is fused into libnerf_hip.so (NeRFModel.forward); it has no eager path")


class ResampleIndexError(RuntimeError):
    """Raised (when ``model.check_resample`` is on) where the reference prints a banner and exit(0)s (nerf.py:251-253)."""


def _call_flags(model, need_grad: bool) -> int:
    bf16 = getattr(model, "bf16_mlp", False)
    # split-fp32: `split_mlp` selects it for inference calls; `split_train` (its own opt-in switch) for TRAINING calls -- forward, dX chain and
    # weight-gradient products on bf16 MFMA with two-part operands (csrc/field_fwd_split.hip, field_bwd_split.hip, dw_bf16.hip's SPLIT form)
    split = (getattr(model, "split_train", False) and not model.force_tile_kernel) if need_grad else getattr(model, "split_mlp", False)
    return ((_abi.SAVE_FOR_BACKWARD if need_grad else 0) | (_abi.FORCE_TILE_KERNEL if model.force_tile_kernel else 0)
            | (_abi.BF16_MLP if bf16 else 0) | (_abi.CORRECTED if getattr(model, "corrected", False) else 0)
            | (_abi.SPLIT_MLP if split and not bf16 else 0))


def _forward_call(model, need_grad, row, col, pb, K9, ray0, params, maps=None, quant=None, dist=None, norm=None):
    """One nerf_hip_forward call on the model's workspace -> (C_coarse, C_fine, ws, flags).  maps ([B, 4] fp32): nerf_hip_forward_maps
    (inference) / nerf_hip_forward_maps_train (need_grad) instead, which also fill maps with each ray's (D_c, A_c, D_f, A_f) and leave the
    colours' bits as they are.  quant = (q, Q) with maps (inference only): nerf_hip_forward_quantiles, which also fills Q ([B, 2, nq] fp32)
    with the quantile depths of the host floats q (rule QD of include/nerf_hip.h) and leaves colours and maps as they are.  dist ([B, 2]
    fp32) with maps (need_grad only): nerf_hip_forward_distortion_train, which also fills dist with each ray's (L_c, L_f) (rule DL).
    norm = (passes, Nrm) with maps (inference only, without quant): nerf_hip_forward_normals on the model's side workspace, which also fills
    the requested rows of Nrm ([B, 2, 3] fp32) with each ray's composited normals (rule NM) and leaves colours and maps as they are."""
    B = row.shape[0]
    Nc, Nf = model.num_coarse, model.num_fine
    flags = _call_flags(model, need_grad)
    ws = model._workspace(B, flags)  # (inside NeRFModel.render: the frame's one workspace, sized for its longest call)
    # rendering loops (`with model.frozen_weights():`): the packed weight image a previous call of the SAME frozen section
    # left in this workspace is reused.  Outside such a section the image is rebuilt on every call (12 us): a version
    # stamp cannot see writes through `.data`, dist.broadcast or raw pointers.
    reuse = model._frozen and not need_grad and (ws.data_ptr(), flags) in model._packed
    call_flags = flags | (_abi.WEIGHTS_UNCHANGED if reuse else 0)
    dev = row.device
    C_c = torch.empty(B, 3, dtype=torch.float32, device=dev)
    C_f = torch.empty(B, 3, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    wptr = _abi.ptr_array(params)
    # the entry and its arguments behind the stream, from the outputs asked for; maps (when asked for) sits in front of the workspace
    lib = _abi.lib()
    if maps is None:
        fn, tail = lib.nerf_hip_forward, ()
    elif quant is not None:
        q, Q = quant
        fn, tail = lib.nerf_hip_forward_quantiles, (_abi.f32_array(q), len(q), Q.data_ptr())
    elif norm is not None:
        passes, Nrm = norm
        nws = model._normals_workspace(B, dev)
        fn, tail = lib.nerf_hip_forward_normals, (passes, Nrm.data_ptr(), nws.data_ptr(), nws.numel())
    elif dist is not None:
        fn, tail = lib.nerf_hip_forward_distortion_train, (dist.data_ptr(),)
    else:
        fn, tail = (lib.nerf_hip_forward_maps_train if need_grad else lib.nerf_hip_forward_maps), ()
    _abi.check(fn(wptr, row.data_ptr(), col.data_ptr(), pb.data_ptr(), K9, ray0, B, Nc, Nf, LAST_DELTA, C_c.data_ptr(), C_f.data_ptr(),
                  *(() if maps is None else (maps.data_ptr(),)), ws.data_ptr(), ws.numel(), call_flags, stream, *tail))
    if model._frozen and not need_grad:
        model._packed.add((ws.data_ptr(), flags))
    model._last_ws = ws
    return C_c, C_f, ws, flags


def _record(ctx, model, flags, ws, B, params, ray0):
    """A training forward on the workspace slot of `flags`: what its backward needs, and the slot's generation (a later training forward on
    the same slot makes this graph's backward raise instead of reading the other call's saves)."""
    gen = model._ws_generation.get(flags, 0) + 1
    model._ws_generation[flags] = gen
    ctx.generation = gen
    ctx.model, ctx.ws, ctx.flags, ctx.B = model, ws, flags, B
    ctx.params, ctx.ray0 = params, ray0
    ctx.bucket = model.grad_bucket  # bound when the graph is recorded: toggling model.grad_bucket later does not change this step


def _backward_call(ctx, call):
    """The shared part of a backward through the library: workspace-generation guard, gradient targets (fresh tensors or the views of
    model.grad_bucket), then `call(ptr_array(params), ptr_array(grads), stream, early_event)`.  Returns the gradients for autograd (None in
    bucket mode, where p.grad IS the bucket view)."""
    model = ctx.model
    if ctx.generation != model._ws_generation.get(ctx.flags):
        raise RuntimeError("the workspace of this forward was reused by a later training forward; call backward first")
    params = ctx.params
    bucket = ctx.bucket
    if bucket is not None:
        # data-parallel trainer: the kernels write straight into views of the flat all-reduce buffer (parallel.GradBucket).
        # Overwrite semantics: ONE backward per step.  torch.autograd.grad, parameter hooks, gradient accumulation and a second
        # loss through the same model are not supported in bucket mode (they would see None / overwritten gradients).
        if len(bucket.params) != len(params) or any(a is not b for a, b in zip(bucket.params, params)):
            raise RuntimeError("model.grad_bucket was built for other parameters")
        if bucket.pending:
            raise RuntimeError("a second backward would overwrite the gradients of the previous one in model.grad_bucket before "
                               "they were used: bucket.allreduce_sum(), train.FusedAdam.step() / .zero_grad() release it; after any other "
                               "optimizer's step call bucket.consume()")
        bucket.pending = True
        grads = bucket.views
    else:
        grads = [torch.empty_like(p) for p in params]
    stream = torch.cuda.current_stream(params[0].device).cuda_stream
    # a bucket with overlap enabled gets the event at which point_layer[0..7]'s gradients are final (parallel.GradBucket)
    early = bucket.early_event_handle if bucket is not None else 0
    call(_abi.ptr_array(params), _abi.ptr_array(grads), stream, early or None)
    if bucket is not None:
        # p.grad IS the bucket view (overwritten every step, like the C ABI's dweights24): nothing for autograd to accumulate
        for p, v in zip(params, grads):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v
        return [None] * len(params)
    return grads


class _RenderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, need_grad, row, col, pb, K9, ray0, *params):
        C_c, C_f, ws, flags = _forward_call(model, need_grad, row, col, pb, K9, ray0, params)
        if need_grad:
            _record(ctx, model, flags, ws, row.shape[0], params, ray0)
        return C_c, C_f

    @staticmethod
    def backward(ctx, dC_c, dC_f):
        dC_c = dC_c.contiguous().float()
        dC_f = dC_f.contiguous().float()
        model = ctx.model
        grads = _backward_call(ctx, lambda wp, gp, stream, early: _abi.check(_abi.lib().nerf_hip_backward_overlap(
            wp, dC_c.data_ptr(), dC_f.data_ptr(), ctx.ray0, ctx.B, model.num_coarse, model.num_fine, LAST_DELTA, gp, ctx.ws.data_ptr(),
            ctx.ws.numel(), ctx.flags, stream, early)))
        return (None, None, None, None, None, None, None, *grads)


class _RenderMapsFn(torch.autograd.Function):
    """A training forward with maps (with_dist False: nerf_hip_forward_maps_train) -> (C_coarse, C_fine, maps [B, 4]), or with maps and the
    distortion loss (with_dist True: nerf_hip_forward_distortion_train) -> (C_coarse, C_fine, maps, dist [B, 2]).  Its backward is ONE
    nerf_hip_backward_maps / nerf_hip_backward_distortion call (DESIGN.md sections 3l, 3m).  An upstream gradient autograd hands over as
    None counts as zero."""

    @staticmethod
    def forward(ctx, model, with_dist, row, col, pb, K9, ray0, *params):
        ctx.set_materialize_grads(False)
        M = torch.empty(row.shape[0], 4, dtype=torch.float32, device=row.device)
        D = torch.empty(row.shape[0], 2, dtype=torch.float32, device=row.device) if with_dist else None
        C_c, C_f, ws, flags = _forward_call(model, True, row, col, pb, K9, ray0, params, maps=M, dist=D)
        _record(ctx, model, flags, ws, row.shape[0], params, ray0)
        ctx.with_dist = with_dist
        return (C_c, C_f, M, D) if with_dist else (C_c, C_f, M)

    @staticmethod
    def backward(ctx, dC_c, dC_f, dM, dD=None):
        B = ctx.B
        dev = ctx.params[0].device
        with_dist = ctx.with_dist
        up = [torch.zeros(B, n, dtype=torch.float32, device=dev) if g is None else g.contiguous().float()
              for g, n in ((dC_c, 3), (dC_f, 3), (dM, 4)) + (((dD, 2),) if with_dist else ())]
        model = ctx.model
        fn = _abi.lib().nerf_hip_backward_distortion if with_dist else _abi.lib().nerf_hip_backward_maps
        grads = _backward_call(ctx, lambda wp, gp, stream, early: _abi.check(fn(
            wp, up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), ctx.ray0, B, model.num_coarse, model.num_fine, LAST_DELTA, gp,
            ctx.ws.data_ptr(), ctx.ws.numel(), ctx.flags, stream, early, *((up[3].data_ptr(),) if with_dist else ()))))
        return (None, None, None, None, None, None, None, *grads)


def field_normals(g):
    """Outward unit normals -g / |g| of sigma gradients g [V, 3] (fp32, |g| = sqrt(g0^2 + g1^2 + g2^2) rounded per operation), (0, 0, 0)
    where |g| is 0 or not finite: the marching-cubes kernel's rule (include/nerf_hip.h)."""
    length = torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])[:, None]
    ok = torch.isfinite(length) & (length > 0)
    return torch.where(ok, -g / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(g))


class _FieldQuery(torch.autograd.Function):
    """NeRFModel.field: forward = nerf_hip_query, backward = nerf_hip_query_grad with the upstream gradients (a recompute; the weights
    are constants).  Outputs (rgb, sigma) with dirs, sigma alone without."""

    @staticmethod
    def forward(ctx, points, model, dirs):
        ctx.model = model
        ctx.save_for_backward(*(t for t in (points, dirs) if t is not None))
        rgb, sigma = model.query(points, dirs)
        return sigma if dirs is None else (rgb, sigma)

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        points, dirs = saved[0], (saved[1] if len(saved) > 1 else None)
        if dirs is None:
            g_rgb, g_sigma = None, grads[0]
        else:
            g_rgb, g_sigma = grads
        if g_sigma is None:
            g_sigma = torch.zeros(points.shape[0], dtype=torch.float32, device=points.device)
        dp = ctx.model.query_grad(points, dirs, dsigma=g_sigma, drgb=g_rgb)[2]
        return dp, None, None


class NeRFModel(nn.Module):
    """Drop-in for the reference's ``NeRFModel`` (nerf.py:169-348)."""

    def __init__(self, num_coarse=64, num_fine=128, batch_ray=8):
        super().__init__()
        self.encoder = Encoder(batch_size=batch_ray)
        self.network = Network(batch_size=batch_ray)
        self.num_coarse = num_coarse
        self.num_fine = num_fine
        self.batch_ray = batch_ray
        #: mimic nerf.py:251-253 (costs one host sync per call, like the reference): raise instead of exit(0)
        self.check_resample = False
        #: (near, far) of the GLOBAL ray 0 when one batch is sharded over several GPUs (quirk Q6); None = local ray 0
        self.ray0_near_far = None
        #: use the LDS-tile field kernels instead of the register-resident ones (A/B measurements, tests)
        self.force_tile_kernel = False
        #: BASELINE.json cfg3: run the MLP on bf16 MFMA (fp32 accumulation, fp32 everything else); ~1e-2 of the fp32 result
        self.bf16_mlp = False
        #: INFERENCE calls (no grad) only: evaluate the fp32 MLP on bf16 MFMA with every fp32 operand split into two bf16 parts (hi + mid)
        #: and three MFMAs per product, fp32 accumulation -- inside the same 1e-4 bar as the exact-fp32 default,
        #: 3x faster.  Off by default: the default keeps exact k-ordered fp32 fma chains; training forwards ignore it (their switch is split_train)
        self.split_mlp = False
        #: TRAINING calls (a forward that records a graph, train_step): the whole train step in split-fp32 arithmetic -- every fp32 operand of
        #: the forward, the dX chain and the weight-gradient products as two bf16 parts (hi + mid), three bf16 MFMAs per product, fp32
        #: accumulation.  Opt-in, never the headline: the default keeps the exact fp32 kernels.  Loss to 1e-5 of the exact path's, gradients
        #: inside the bands the exact path is held to against the reference (tests/test_gpu_split.py)
        self.split_train = False
        #: OPTIONAL EXTRA, off by default, NOT the reference's results (SURVEY.md 8a "Q"): one stable sort of the merged samples by depth with
        #: rgb / sigma moving along (instead of nerf.py:307-308's five independent channel sorts) and a detached t_fine (instead of
        #: nerf.py:259's attached one).  Parity unpinned -- the reference has no such mode; tested against the oracle's restatement only
        self.corrected = False
        #: parallel.GradBucket or None.  When set (read when the forward records the graph), backward writes the 24 gradients straight
        #: into the bucket's flat buffer and makes p.grad its views (overwrite semantics: one backward per step, a second one before
        #: the gradients were consumed raises; autograd.grad / hooks unsupported), so the all-reduce needs no pack / unpack
        self.grad_bucket = None
        self._ws_capacity = False  # True inside render(): an inference slot sized for more rays serves shorter calls too
        self._ws = {}            # flags -> (key, workspace): one slot per flag set (training / inference / bf16 ...)
        self._ws_generation = {}  # flags -> count of training forwards on that slot
        self._last_ws = None
        self._frozen = False
        self._packed = set()
        self._qws = {}           # with_rgb -> workspace of the point queries (query / density_grid): independent of the point count
        self._nws = None         # (key, side workspace) of the normal-map calls (render(normals=)): one slot, replaced when its sizes change

    # ----- plumbing -------------------------------------------------------------------------
    def _workspace(self, B, flags):
        """One workspace per flag set, so that a validate-while-training loop (17 GB training workspace at cfg2 + a small
        inference one) does not reallocate on every switch; a slot is replaced when its sizes or device change."""
        dev = self.network.point_info.weight.device
        key = (B, self.num_coarse, self.num_fine, flags, dev)
        slot = self._ws.get(flags)
        if slot is not None and self._ws_capacity and slot[0][1:] == key[1:] and slot[0][0] >= B and not (flags & _abi.SAVE_FOR_BACKWARD):
            return slot[1]  # NeRFModel.render: calls of different lengths share the slot sized for the longest one (the regions in
            #                 front of the per-ray ones -- status, packed weight images -- do not move with B: csrc/api.hip layout())
        if slot is None or slot[0] != key:
            self._ws.pop(flags, None)
            slot = None
            n = _abi.ws_bytes(B, self.num_coarse, self.num_fine, flags)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            assert ws.data_ptr() % 256 == 0
            ws[:256].zero_()  # the status region: its sticky word is the caller's to initialise (nerf_hip_read_status_sticky)
            self._ws[flags] = slot = (key, ws)
            self._packed = {k for k in self._packed if k[1] != flags}
        return slot[1]

    def _normals_workspace(self, B, dev):
        """The side workspace of nerf_hip_forward_normals: one slot, replaced when its sizes or device change; inside render() the slot
        sized for the longest call serves the shorter ones too (the library carves it for the call's own B)."""
        key = (B, self.num_coarse, self.num_fine, dev)
        slot = self._nws
        if slot is not None and (slot[0] == key or (self._ws_capacity and slot[0][1:] == key[1:] and slot[0][0] >= B)):
            return slot[1]
        self._nws = None
        nws = torch.empty(_abi.normals_ws_bytes(B, self.num_coarse, self.num_fine), dtype=torch.uint8, device=dev)
        assert nws.data_ptr() % 256 == 0
        self._nws = (key, nws)
        return nws

    @property
    def last_workspace(self):
        """The workspace the most recent forward ran on (introspection: _abi.ws_view, status word)."""
        return self._last_ws

    @contextlib.contextmanager
    def frozen_weights(self):
        """Rendering loops: inside this section the caller guarantees that no parameter is written, so the packed weight
        image is built once per workspace and reused (NERF_HIP_WEIGHTS_UNCHANGED) instead of rebuilt on every call.
        Opt-in because no stamp can see every write (``p.data.add_()``, ``dist.broadcast(p.data)``, raw pointers)."""
        prev = self._frozen
        self._frozen = True
        if not prev:
            self._packed = set()
        try:
            yield self
        finally:
            self._frozen = prev
            if not prev:
                self._packed = set()

    def __getstate__(self):  # torch.save(model) (nerf.py:491) must not pickle the workspace
        d = dict(self.__dict__)
        d["_ws"] = {}
        d["_ws_generation"] = {}
        d["_last_ws"] = None
        d["_packed"] = set()
        d["_frozen"] = False
        d["_ws_capacity"] = False
        d["grad_bucket"] = None
        d["_qws"] = {}
        d["_nws"] = None
        return d

    def __setstate__(self, d):  # checkpoints written by an earlier build lack the newer plumbing attributes
        super().__setstate__(d)
        self.__dict__.setdefault("grad_bucket", None)
        self.__dict__.setdefault("split_mlp", False)
        self.__dict__.setdefault("split_train", False)
        self.__dict__.setdefault("corrected", False)
        self.__dict__["_ws"], self.__dict__["_ws_generation"] = {}, {}
        self.__dict__["_last_ws"], self.__dict__["_packed"], self.__dict__["_frozen"] = None, set(), False
        self.__dict__["_ws_capacity"] = False
        self.__dict__["_qws"] = {}
        self.__dict__["_nws"] = None

    def _params(self):
        ps = list(self.network.parameters())
        for p in ps:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise RuntimeError("network parameters must be contiguous fp32")
        return ps

    # ----- reference surface ----------------------------------------------------------------
    def ray_loss(self, C_coarse, C_fine, C_true):
        """nerf.py:325-331: sum (not mean) of squared errors of both colours."""
        return _RayLossFn.apply(C_coarse, C_fine, C_true)

    def mask_loss(self, maps, alpha):
        """Not in the reference: the alpha-mask loss of object captures, sum_b (A_c,b - alpha_b)^2 + (A_f,b - alpha_b)^2 over the opacity
        columns of forward(maps=True)'s maps [B, 4] and the batch's alpha [B] -- a sum, like ray_loss.  Plain torch ops on B elements."""
        a = alpha.reshape(-1).to(maps.device, torch.float32)
        return torch.sum(torch.square(maps[:, 1] - a)) + torch.sum(torch.square(maps[:, 3] - a))

    def distortion_loss(self, dist, coarse=False):
        """Not in the reference: the distortion loss of mip-NeRF 360 over a batch, sum_b L_f,b (coarse=True: + sum_b L_c,b) of
        forward(maps=True, distortion=True)'s dist [B, 2] (rule DL of include/nerf_hip.h) -- a sum, like ray_loss.  Plain torch ops on B
        elements."""
        loss = torch.sum(dist[:, 1])
        return loss + torch.sum(dist[:, 0]) if coarse else loss

    def forward(self, row, column, poses_bound, K_inv, maps=False, distortion=False):
        """nerf.py:333-348.  row/column [B] i64, poses_bound [B,17] (any float dtype), K_inv [3,3];
        CPU or device tensors.  Returns (C_coarse, C_fine) [B,3] fp32 on the model's device.
        maps=True (not in the reference): returns (C_coarse, C_fine, maps) with maps [B, 4] = each ray's (D_c, A_c, D_f, A_f), expected depth
        and accumulated opacity of the coarse and the fine composite (include/nerf_hip.h).  With grad enabled and a parameter that requires
        grad the call records a graph and all three outputs are differentiable with respect to the weights (a mask or depth loss:
        DESIGN.md section 3l); otherwise it is the inference maps call.  The colours' bits are those of maps=False either way.
        distortion=True (with maps=True, training only): returns (C_coarse, C_fine, maps, dist) with dist [B, 2] = each ray's distortion
        loss (L_c, L_f) of the coarse and the fine pass (rule DL of include/nerf_hip.h), differentiable with the rest (DESIGN.md section
        3m); colours and maps keep their bits.  ValueError before any device work without maps=True or where no graph would be recorded."""
        if distortion and not maps:
            raise ValueError("distortion=True needs maps=True: the distortion loss comes with the training maps call")
        if distortion and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.network.parameters())):
            raise ValueError("distortion=True is a training output: grad is disabled or no parameter requires grad, so no graph would be "
                             "recorded; render(quantiles=) is the inference-time view of the same spread")
        ps = self._params()
        dev = ps[0].device
        if dev.type != "cuda":
            raise RuntimeError("NeRFModel runs only on a ROCm device (MI355X): model.to('cuda'); there is no CPU path")
        if row.shape[0] != self.batch_ray:
            raise ValueError(f"batch of {row.shape[0]} rays, model built for batch_ray={self.batch_ray} (nerf.py:172-176)")
        return self._launch(ps, row, column, poses_bound, K_inv, maps=maps, train_maps=maps, distortion=distortion)

    def _launch(self, ps, row, column, poses_bound, K_inv, maps=False, train_maps=False, quantiles=None, distortion=False, normals=0):
        """maps=True: nerf_hip_forward_maps, -> (C_coarse, C_fine, maps [B, 4]) -- with no graph unless `train_maps` is set and grad is
        enabled for a parameter (then nerf_hip_forward_maps_train under _RenderMapsFn).  quantiles (a tuple of floats; maps=True, never
        recorded): nerf_hip_forward_quantiles, -> (C_coarse, C_fine, maps, Q [B, 2, nq]).  distortion (forward has checked that a graph is
        recorded): nerf_hip_forward_distortion_train under _RenderMapsFn too, -> (C_coarse, C_fine, maps, dist [B, 2]).  normals (the passes of
        rule NM, bit 0 coarse, bit 1 fine; maps=True, never recorded): nerf_hip_forward_normals, with Nrm [B, 2, 3] appended to the return --
        rows not asked for NaN; with quantiles too, a quantile call runs on the same rays first, for Q alone (same colour and maps bits)."""
        dev = ps[0].device
        K9 = _abi.f32_array(K_inv.detach().to("cpu", torch.float32).reshape(-1).tolist())
        pb = poses_bound.to(torch.float).to(dev).contiguous()  # cast first like nerf.py:338
        row_d = row.to(dev, torch.int64).contiguous()
        col_d = column.to(dev, torch.int64).contiguous()
        ray0 = _abi.f32_array(self.ray0_near_far) if self.ray0_near_far is not None else None
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in ps)  # grad mode is off inside Function.forward
        Q = None
        if distortion:
            C_c, C_f, M, Q = _RenderMapsFn.apply(self, True, row_d, col_d, pb, K9, ray0, *ps)  # (the fourth output: dist here, the quantile depths below)
        elif maps and train_maps and need_grad:
            C_c, C_f, M = _RenderMapsFn.apply(self, False, row_d, col_d, pb, K9, ray0, *ps)
        elif maps:
            M = torch.empty(row_d.shape[0], 4, dtype=torch.float32, device=dev)
            if quantiles is not None:
                Q = torch.empty(row_d.shape[0], 2, len(quantiles), dtype=torch.float32, device=dev)
            Nrm = torch.full((row_d.shape[0], 2, 3), float("nan"), dtype=torch.float32, device=dev) if normals else None
            with torch.no_grad():
                if quantiles is not None or not normals:
                    C_c, C_f, _, _ = _forward_call(self, False, row_d, col_d, pb, K9, ray0, ps, maps=M,
                                                   quant=None if quantiles is None else (quantiles, Q))
                if normals:
                    C_c, C_f, _, _ = _forward_call(self, False, row_d, col_d, pb, K9, ray0, ps, maps=M, norm=(normals, Nrm))
            if Nrm is not None:
                if self.check_resample and self.resample_fault():
                    raise ResampleIndexError("resample index outside [0, Nf-1] (the reference exit(0)s here, nerf.py:251-253)")
                return (C_c, C_f, M, Nrm) if Q is None else (C_c, C_f, M, Q, Nrm)
        else:
            C_c, C_f = _RenderFn.apply(self, need_grad, row_d, col_d, pb, K9, ray0, *ps)
        if self.check_resample and self.resample_fault():
            raise ResampleIndexError("resample index outside [0, Nf-1] (the reference exit(0)s here, nerf.py:251-253)")
        if Q is not None:
            return C_c, C_f, M, Q
        return (C_c, C_f, M) if maps else (C_c, C_f)

    def train_step(self, row, column, poses_bound, K_inv, C_true):
        """The device work of one iteration of the reference's loop (nerf.py:470-473: ``model(...)``, ``ray_loss``, ``loss.backward()``) in ONE
        library call (``nerf_hip_train_step``): the same kernels enqueued back to back without the interpreter between them -- at a 400 / 512-ray
        batch three separate calls leave 3 % of the step in gaps.  Leaves the gradients of this batch in ``p.grad`` exactly as the autograd
        path does -- fresh tensors, or the views of ``model.grad_bucket`` (overwrite semantics, ``pending`` set) -- and returns
        ``(C_coarse, C_fine, loss)`` (detached; ``loss`` a 0-dim tensor).  Bit-identical to the three calls
        (tests/test_gpu_train.py::test_fused_train_step_equals_autograd_path).  What ``NeRFRunner.trainer`` calls."""
        ps = self._params()
        dev = ps[0].device
        if dev.type != "cuda":
            raise RuntimeError("NeRFModel runs only on a ROCm device (MI355X): model.to('cuda'); there is no CPU path")
        if row.shape[0] != self.batch_ray:
            raise ValueError(f"batch of {row.shape[0]} rays, model built for batch_ray={self.batch_ray} (nerf.py:172-176)")
        B, Nc, Nf = row.shape[0], self.num_coarse, self.num_fine
        K9 = _abi.f32_array(K_inv.detach().to("cpu", torch.float32).reshape(-1).tolist())
        pb = poses_bound.to(torch.float).to(dev).contiguous()
        row_d, col_d = row.to(dev, torch.int64).contiguous(), column.to(dev, torch.int64).contiguous()
        Ct = C_true.to(dev, torch.float32).contiguous()
        ray0 = _abi.f32_array(self.ray0_near_far) if self.ray0_near_far is not None else None
        flags = _call_flags(self, True)
        ws = self._workspace(B, flags)
        bucket = self.grad_bucket
        if bucket is not None:
            if len(bucket.params) != len(ps) or any(a is not b for a, b in zip(bucket.params, ps)):
                raise RuntimeError("model.grad_bucket was built for other parameters")
            if bucket.pending:
                raise RuntimeError("a second backward would overwrite the gradients of the previous one in model.grad_bucket before "
                                   "they were used: bucket.allreduce_sum(), train.FusedAdam.step() / .zero_grad() release it; after any other "
                                   "optimizer's step call bucket.consume()")
            bucket.pending = True
            grads = bucket.views
        else:
            grads = [torch.empty_like(p) for p in ps]
        C_c = torch.empty(B, 3, dtype=torch.float32, device=dev)
        C_f = torch.empty(B, 3, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        early = bucket.early_event_handle if bucket is not None else 0
        _abi.check(_abi.lib().nerf_hip_train_step(_abi.ptr_array(ps), row_d.data_ptr(), col_d.data_ptr(), pb.data_ptr(), K9, ray0, Ct.data_ptr(),
                                                  B, Nc, Nf, LAST_DELTA, C_c.data_ptr(), C_f.data_ptr(), loss.data_ptr(), _abi.ptr_array(grads),
                                                  ws.data_ptr(), ws.numel(), flags, torch.cuda.current_stream(dev).cuda_stream, early or None))
        self._last_ws = ws
        self._ws_generation[flags] = self._ws_generation.get(flags, 0) + 1  # a graph recorded earlier on this slot is stale now
        for p, g in zip(ps, grads):
            if bucket is not None:
                if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                    p.grad = g
            else:
                p.grad = g  # overwrite, like zero_grad(set_to_none=True); backward()
        if self.check_resample and self.resample_fault():
            raise ResampleIndexError("resample index outside [0, Nf-1] (the reference exit(0)s here, nerf.py:251-253)")
        return C_c, C_f, loss.reshape(())

    def resample_fault(self) -> bool:
        """Did the most recent forward meet the reference's exit condition -- a ray whose resampling index falls outside [0, Nf-1], i.e.
        whose coarse weights all vanished (nerf.py:251-253: banner + exit(0))?  The device path clamps the index and goes on; this reads
        the status word the kernels left (ONE host sync)."""
        return bool(self.read_status() & _abi.STATUS_RESAMPLE_INDEX)

    def read_status(self) -> int:
        """The status word of the most recent call on this model (``nerf_hip_read_status``: ONE host sync).  Raises ``NerfHipError`` on
        STATUS_PREP_TIMEOUT -- the one-launch preparation of a bf16-MLP call gave up waiting for its weight fold, the packed weight image
        is poisoned with NaN and so are the outputs of every call that used it (csrc/prep_bf16.hip) -- so that no caller renders or trains
        on from there."""
        ws = self._last_ws
        if ws is None:
            return 0
        st = C.c_uint32(0)
        _abi.check(_abi.lib().nerf_hip_read_status(ws.data_ptr(), ws.numel(), C.byref(st), torch.cuda.current_stream(ws.device).cuda_stream))
        if st.value & _abi.STATUS_PREP_TIMEOUT:
            raise _abi.NerfHipError("a bf16-MLP call's one-launch preparation gave up waiting for the weight fold (prep_bf16.hip): the packed weight "
                                    "image is poisoned, the outputs of that call are NaN")
        return int(st.value)

    def resample_fault_since(self, clear: bool = True) -> bool:
        """Did ANY forward on the current workspaces meet that condition since the last call that cleared the record?  The kernels OR the
        status bits into a sticky word no forward resets (``nerf_hip_read_status_sticky``), so a train loop that looks only at its logging
        points misses nothing in between -- the reference checks every forward (nerf.py:251-253).  One host sync per workspace."""
        hit = timeout = False
        for _, ws in self._ws.values():  # every workspace is read (and cleared) before anything is raised
            st = C.c_uint32(0)
            _abi.check(_abi.lib().nerf_hip_read_status_sticky(ws.data_ptr(), ws.numel(), C.byref(st), 1 if clear else 0,
                                                              torch.cuda.current_stream(ws.device).cuda_stream))
            timeout = timeout or bool(st.value & _abi.STATUS_PREP_TIMEOUT)
            hit = hit or bool(st.value & _abi.STATUS_RESAMPLE_INDEX)
        if timeout:
            raise _abi.NerfHipError("a bf16-MLP call's one-launch preparation gave up waiting for the weight fold (prep_bf16.hip): the packed "
                                    "weight image of that call was poisoned, its results are NaN")
        return hit

    # ----- the field at explicit points (not in the reference: what a trained model is queried for besides rendering) ---------------------
    def _query_workspace(self, with_rgb: bool, dev):
        ws = self._qws.get(with_rgb)
        if ws is None or ws.device != dev:
            ws = torch.empty(_abi.query_ws_bytes(with_rgb), dtype=torch.uint8, device=dev)
            self._qws[with_rgb] = ws
        return ws

    @torch.no_grad()
    def query(self, points, dirs=None):
        """The field (Network + Encoder, nerf.py:101-124, 135-167) at explicit points: points [M, 3] world coordinates, any M (0 too);
        dirs [M, 3] unit world directions as Encoder consumes them (not renormalised) or None.  Returns (rgb [M, 3] or None, sigma [M]),
        fp32 on the model's device, not requiring grad; the weights are only read.  ALWAYS exact fp32 -- ``bf16_mlp`` / ``split_mlp``
        do not apply -- and bit-identical to what a forward computes for a sample at the same point seen along the same direction.
        Without dirs only sigma is computed (the colour branch is skipped).  Accurate for |p| <= 320 per coordinate
        (include/nerf_hip.h)."""
        from . import ops

        ps = self._params()
        dev = ps[0].device
        if dev.type != "cuda":
            raise RuntimeError("NeRFModel runs only on a ROCm device (MI355X): model.to('cuda'); there is no CPU path")
        pts = torch.as_tensor(points).to(dev, torch.float32).reshape(-1, 3)
        d = torch.as_tensor(dirs).to(dev, torch.float32).reshape(-1, 3) if dirs is not None else None
        return ops.query(ps, pts, d, ws=self._query_workspace(d is not None, dev))

    def _query_grad_workspace(self, with_rgb: bool, dev):
        key = ("grad", with_rgb)
        ws = self._qws.get(key)
        if ws is None or ws.device != dev:
            ws = torch.empty(_abi.query_grad_ws_bytes(with_rgb), dtype=torch.uint8, device=dev)
            self._qws[key] = ws
        return ws

    def _device_params(self):
        ps = self._params()
        if ps[0].device.type != "cuda":
            raise RuntimeError("NeRFModel runs only on a ROCm device (MI355X): model.to('cuda'); there is no CPU path")
        return ps

    @torch.no_grad()
    def query_grad(self, points, dirs=None, dsigma=None, drgb=None):
        """query() and the vector-Jacobian product of the field with respect to the points: points [M, 3], dirs [M, 3] or None as in
        query(); upstream dsigma [M] (None = ones, which gives the gradient of sigma) and, only with dirs, drgb [M, 3] (None = no colour
        term).  Returns (rgb [M, 3] or None, sigma [M], dpoints [M, 3]) with dpoints[m] = dsigma[m] d sigma_m / d p_m + drgb[m] . d rgb_m
        / d p_m.  rgb and sigma are query()'s bits.  Exact fp32 whatever ``bf16_mlp`` / ``split_mlp`` say; gradients with respect to
        points only (not dirs, not the weights).  The gradient convention is the train step's (include/nerf_hip.h): the encoding's
        phase fp32(x * f) is differentiated as if it were exact, and d|s|/ds = sign(s) with sign(0) = 0."""
        from . import ops

        ps = self._device_params()
        dev = ps[0].device
        pts = torch.as_tensor(points).to(dev, torch.float32).reshape(-1, 3)
        d = torch.as_tensor(dirs).to(dev, torch.float32).reshape(-1, 3) if dirs is not None else None
        ds = torch.as_tensor(dsigma).to(dev, torch.float32).reshape(-1) if dsigma is not None else None
        dc = torch.as_tensor(drgb).to(dev, torch.float32).reshape(-1, 3) if drgb is not None else None
        return ops.query_grad(ps, pts, d, ds, dc, ws=self._query_grad_workspace(d is not None, dev))

    def field(self, points, dirs=None):
        """query() as a differentiable function of the points: returns (rgb [M, 3] or None, sigma [M]) with query()'s values, and a
        backward that runs nerf_hip_query_grad with the upstream gradients (recomputing the forward: nothing per point is kept between
        the two).  The gradient flows to ``points`` only: the weights are constants of this function (they get no .grad from it, and
        must not change between forward and backward), and ``dirs`` must not require grad -- no gradient with respect to directions is
        computed, so that raises instead of silently giving none.  For surface normals, eikonal or surface-projection losses and probes."""
        if dirs is not None and torch.is_tensor(dirs) and dirs.requires_grad:
            raise ValueError("model.field gives gradients with respect to points only: dirs must not require grad (detach them)")
        ps = self._device_params()
        dev = ps[0].device
        pts = torch.as_tensor(points).to(dev, torch.float32).reshape(-1, 3)
        d = torch.as_tensor(dirs).to(dev, torch.float32).reshape(-1, 3).detach() if dirs is not None else None
        if d is None:
            return None, _FieldQuery.apply(pts, self, None)
        rgb, sigma = _FieldQuery.apply(pts, self, d)
        return rgb, sigma

    @torch.no_grad()
    def density_grid(self, lo, hi, res):
        """sigma on a regular lattice spanning the box [lo, hi] (three floats each): res = n or (nx, ny, nz), every n >= 1 and
        nx * ny * nz < 2^31.  Point (i, j, k) is lo + (i, j, k) * step with step = (hi - lo) / (n - 1) computed in fp32 on the host
        (0 where n == 1), each coordinate one fp32 product and one fp32 sum -- so the LAST point is lo + (n - 1) * step, which can
        differ from hi in the last bits.  Returns sigma [nx, ny, nz] (C order, z fastest) on the model's device, exact fp32 whatever
        ``bf16_mlp`` / ``split_mlp`` say, and no points buffer is formed: a 512^3 grid needs its 512 MiB of sigma and nothing else."""
        import numpy as np

        from . import ops

        ps = self._params()
        dev = ps[0].device
        if dev.type != "cuda":
            raise RuntimeError("NeRFModel runs only on a ROCm device (MI355X): model.to('cuda'); there is no CPU path")
        shape = grid_shape(res)
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        step = grid_step(lo32, hi32, shape)
        return ops.density_grid(ps, lo32.tolist(), step.tolist(), shape, ws=self._query_workspace(False, dev))

    @torch.no_grad()
    def density_band(self, lo, hi, res, level, block=8):
        """density_grid(lo, hi, res) with the field evaluated only near the level set sigma == level: a coarse pass samples the corners
        of blocks of ``block``^3 lattice points (block >= 2), and the exact field is evaluated in a band of blocks around the corners'
        class changes that grows until the surface no longer leaves it.  Returns (sigma [nx, ny, nz], info).  Every evaluated value is
        density_grid's, bit for bit; every other point holds its block's lowest corner value, which has the right class.  Marching
        cubes at ``level`` over this array therefore gives the dense mesh restricted to the cells the band reached -- the dense mesh
        itself, bit for bit, when every connected piece of the surface shows in some block's corner samples or hangs together with
        one that does.  WHAT IT CANNOT SEE: a piece that fits between the corner samples (an island smaller than a block, a whole
        object inside one block) is missing, silently: lower ``block`` where that matters, or use density_grid.  info: ``rounds`` (grow
        iterations), ``blocks_active``, ``blocks_total``, ``points_evaluated`` (the unique corner points plus the points of every block
        as it becomes active, so corner points inside active blocks count twice) and ``points_total``.  Exact fp32 whatever
        ``bf16_mlp`` / ``split_mlp`` say; the array is for this level only."""
        import numpy as np

        from . import ops

        ps = self._device_params()
        dev = ps[0].device
        shape = grid_shape(res)
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        step = grid_step(lo32, hi32, shape)
        ws = torch.empty(_abi.band_ws_bytes(*shape, int(block)), dtype=torch.uint8, device=dev)
        return ops.density_band(ps, lo32.tolist(), step.tolist(), shape, level, block, ws=ws)

    @torch.no_grad()
    def bake_volume(self, lo, hi, res, degree=2, sigma_min=0.0, block=8, points_per_call=1 << 22, compact=None):
        """The field baked into an SH radiance volume (volume.Volume; rules VA, VS and VO of include/nerf_hip.h) over the lattice of
        density_grid(lo, hi, res), every n >= 2: sigma is density_grid's, with values below ``sigma_min`` set to 0; the ACTIVE points --
        those a lookup with a positive sigma can read -- get the (degree + 1)^2 real spherical-harmonic coefficients of their colour,
        projected through the 12 directions of the icosahedron: per chunk of at most ``points_per_call`` active points and per
        direction, points -> query -> accumulate; every other point keeps 0.  ``block``: cells per edge of the marcher's occupancy
        blocks.  Always exact fp32 whatever ``bf16_mlp`` / ``split_mlp`` say, and bit-identical for every ``points_per_call``; a
        lower-degree bake is the leading slab of the degree-2 bake.  sigma_min = 0 keeps everything the field calls dense, its fog
        included.  Dense storage: 4 + 12 (degree + 1)^2 bytes per lattice point.
        compact = "fp32" / "fp16": a volume.CompactVolume (rule VC) instead -- the SH terms are accumulated straight into the rows of
        the active points (the same accumulate call on the rows seen as a small lattice of their own) and, for "fp16", converted at
        the end; the dense coefficient array is never allocated.  Bit for bit volume.pack(bake_volume(...), compact)."""
        import numpy as np

        from . import ops, volume

        ps = self._device_params()
        dev = ps[0].device
        shape = grid_shape(res)
        if min(shape) < 2:
            raise ValueError(f"res {res!r}: a volume has at least 2 points per axis")
        if degree not in (0, 1, 2):
            raise ValueError(f"degree={degree!r}: 0, 1 or 2")
        if int(points_per_call) != points_per_call or int(points_per_call) < 1:
            raise ValueError(f"points_per_call={points_per_call!r}: an int >= 1")
        if compact not in (None, "fp32", "fp16"):
            raise ValueError(f"compact={compact!r}: None, 'fp32' or 'fp16'")
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        step = grid_step(lo32, hi32, shape)
        sigma = self.density_grid(lo32, hi32, shape)
        if float(sigma_min) != 0.0:
            sigma = torch.where(sigma >= float(sigma_min), sigma, torch.zeros_like(sigma))
        index = ops.volume_active(sigma)
        ncoef = (int(degree) + 1) ** 2
        n = int(index.shape[0])
        if compact is None:
            coef = torch.zeros(*shape, ncoef, 3, device=dev)
        else:
            # the rows as a lattice of their own for the accumulate and convert calls, which want two points per axis: (n4 / 4, 2, 2),
            # n4 = n rounded up to a multiple of 4 and at least 8 -- at most 7 rows more than n, and the calls' bounds are the allocation's
            n4 = max(8, (n + 3) // 4 * 4)
            coef = torch.zeros(n4 // 4, 2, 2, ncoef, 3, device=dev)
        dirs = torch.from_numpy(volume.sh_dirs()).to(dev)
        ws = self._query_workspace(True, dev)
        per = int(points_per_call)
        for p0 in range(0, n, per):
            idx = index[p0:p0 + per]
            pts = ops.volume_points(idx, shape, lo32.tolist(), step.tolist())
            rows = idx if compact is None else torch.arange(p0, p0 + int(idx.shape[0]), dtype=torch.int32, device=dev)
            for k in range(dirs.shape[0]):
                rgb, _ = ops.query(ps, pts, dirs[k].expand(pts.shape[0], 3).contiguous(), ws=ws)
                ops.volume_sh_accumulate(coef, rows, rgb, k)
        occ = ops.volume_blocks(sigma, block)
        if compact is None:
            return volume.Volume(sigma, coef, occ, lo32, step, min(int(block), volume.ONE_BLOCK), int(degree))
        slot = ops.volume_compact_slots(index, shape)
        sigma_rows = sigma.reshape(-1)[index.long()]
        if compact == "fp16":
            _, coef = ops.volume_compact_pack(None, coef, None, True)
        coef_rows = coef.reshape(n4, -1)[:n]
        return volume.CompactVolume(slot, sigma_rows, coef_rows, occ, lo32, step, min(int(block), volume.ONE_BLOCK), int(degree), tuple(shape))

    @torch.no_grad()
    def extract_mesh(self, lo, hi, res, level, color=True, normals="grid", band=None, min_faces=None, keep_largest=None, simplify=None,
                     smooth=None, visible=None, texture=None):
        """A triangle mesh of the isosurface sigma == level over the box [lo, hi]: density_grid(lo, hi, res) -> mesh.marching_cubes (the
        grid's lattice, inside = sigma > level) -> with color, query(verts, dirs=-normals), the colour a ray looking at the surface along
        its inward normal sees.  Returns mesh.Mesh(verts [V, 3], faces [F, 3] int32, normals [V, 3], rgb [V, 3] or None) on the model's
        device, exact fp32 whatever ``bf16_mlp`` / ``split_mlp`` say.  The grid's 4 bytes per point are held only during the call, with
        a mesh workspace of 4 bytes per point more.
        normals="grid": the marching-cubes normals (central differences of the grid, interpolated to the vertex).  normals="field": -g / |g|
        of the field's analytic gradient g at each vertex (query_grad; (0, 0, 0) where |g| is 0 or not finite) -- not limited by the grid
        spacing; the colours are then seen along these normals.
        band=None: the dense grid.  band=r (an int >= 2): density_band(lo, hi, res, level, block=r) in its place -- the field is evaluated
        only in blocks of r^3 points around the surface, and the mesh is the dense one wherever the band found the surface; a component
        smaller than a block can be missed (density_band says when).  Everything after the grid is the same.
        min_faces=n / keep_largest=k (either or both; None, None: nothing of this runs): the floaters go -- right after marching cubes
        the mesh's connected components are labelled on the device (mesh.components) and only those with at least n faces and, with k,
        among the k with the most faces stay (mesh.select_components, mesh.filter_components).  This happens BEFORE the field normals and
        the colours are queried, so a dropped vertex is never evaluated; the result is, bit for bit, filter_components applied to the
        unfiltered call.  With band=: the band may already have missed islands smaller than a block; filtering removes the rest.
        simplify=None: nothing more.  simplify=k (an int >= 2): the mesh is simplified on the device by vertex clustering in cells of k
        lattice steps (mesh.simplify with lo = the grid's lo, cell = fp32(k * step) -- 1 along an axis of one lattice point -- and
        dims = max(1, ceil((n - 1) / k)) per axis): a mesh of roughly 1 / k^2 of the faces.  It runs after marching cubes and after the
        component filter (min_faces still counts the original faces) and BEFORE the field normals and the colours, which are then
        queried at the new vertices only; with normals="grid" the normals are the clusters' summed and normalised grid normals.  The
        result is, bit for bit, mesh.simplify of the unsimplified call's mesh with normals and colours made at its vertices.
        smooth=None: nothing more, and every output keeps its bits.  smooth=n (an int >= 1): n Taubin iterations on the device
        (mesh.smooth with its default weights and pinned boundary, lo = the grid's lo and scale = mesh.pow2_at_least of the grid box's
        largest fp32 extent) take the lattice staircase and the field's noise out of the positions.  It runs AFTER the component filter
        and BEFORE simplify, so simplification clusters the denoised surface; with normals="grid" the normals are then mesh.smooth's
        (area-weighted, from the faces) -- averaged per cluster by simplify --, with normals="field" they are the field's gradient at
        the final vertices as always.  The result is, bit for bit, the later stages applied to mesh.smooth of the earlier stages' mesh.
        visible=None: nothing more.  visible=(poses_bound [n, 17], K_inv, H, W): the faces that none of these cameras sees go, with the
        vertices only they use -- interior sheets and pockets of the isosurface that hang on to the object, which the component filter
        cannot drop (mesh.visibility with its default tmin: one shadow ray from each face's centroid to each camera, on the device;
        then mesh.filter_faces).  It runs AFTER the component filter and BEFORE smoothing, simplification and the normal and colour
        queries, so a hidden vertex is never evaluated.  With normals="grid" the kept vertices keep their grid normals.  The result
        is, bit for bit, the later stages applied to mesh.filter_faces of the earlier stages' mesh.
        texture=None: nothing more.  texture=S (an int, with color): a texture atlas of at most S x S texels is baked for the FINAL mesh
        -- after every stage above, the normals and the colours -- with the chart mesh.atlas_chart(F, S): the field is queried at every
        texel's surface point along its inward normal (bake_texture below), and the mesh.Texture is kept as ``self.last_texture``;
        its corner texels are the vertex colours, bit for bit.  The returned Mesh is the one the call without texture returns."""
        import numpy as np

        from . import mesh

        _check_mesh_stages(normals, simplify, smooth)
        shape = grid_shape(res)
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        sigma = self.density_grid(lo32, hi32, shape) if band is None else self.density_band(lo32, hi32, shape, level, block=band)[0]
        verts, faces, nrm = mesh.marching_cubes(sigma, level, lo32, grid_step(lo32, hi32, shape))
        del sigma
        return self._mesh_stages(verts, faces, nrm, lo32, hi32, shape, color, normals, min_faces, keep_largest, simplify, smooth, visible,
                                 texture=texture)

    @torch.no_grad()
    def bake_texture(self, m, chart, rows_per_call=None):
        """A mesh.Texture of the Mesh m (with normals) with charts of ``chart`` texels, shaded by the field: mesh.bake_texture with
        shade = query(points, dirs)[0] -- at every texel the colour a ray looking at the surface along its inward normal sees, the
        colour extract_mesh gives the vertices; exact fp32 whatever ``bf16_mlp`` / ``split_mlp`` say.  The view direction is fixed to
        the inward normal: view-dependent effects are baked as seen from straight ahead."""
        from . import mesh

        return mesh.bake_texture(m, chart, lambda p, d: self.query(p, d)[0], rows_per_call)

    def _mesh_stages(self, verts, faces, nrm, lo32, hi32, shape, color, normals, min_faces, keep_largest, simplify, smooth, visible, fused=None,
                     texture=None):
        """Everything of extract_mesh / extract_mesh_tsdf behind marching cubes, in extract_mesh's documented order: the component
        filter, the visibility filter, smoothing, simplification, then the field normals and the colours at the final vertices.
        verts / faces / nrm: marching cubes' output over the lattice (lo32, hi32, shape).  fused: None, or a colour volume over that
        lattice (mesh.tsdf_color_volume's C) -- with color, the colours are then mesh.tsdf_sample_color(C) at the final vertices, the
        field is queried only at the vertices that have no fused colour, and ``self.last_fused_fallback`` is their number.
        texture: None, or the bound S on the atlas's edge -- with color, the final mesh is baked with the chart mesh.atlas_chart(F, S)
        from the source of the vertex colours (the fused volume where it has a colour, the field elsewhere) into
        ``self.last_texture``."""
        from . import mesh

        if texture is not None and not color:
            raise ValueError("texture= bakes colours: it needs color")

        if min_faces is not None or keep_largest is not None:
            comps = mesh.components(faces, len(verts), verts)
            keep = mesh.select_components(comps, 1 if min_faces is None else min_faces, keep_largest)
            verts, faces, nrm, _ = mesh.filter_components(mesh.Mesh(verts, faces, None if normals == "field" else nrm, None), comps, keep)
        if visible is not None:
            poses_bound, K_inv, H, W = visible
            m = mesh.Mesh(verts, faces, None if normals == "field" else nrm, None)
            self.last_visibility = mesh.visibility(m, poses_bound, K_inv, H, W)
            verts, faces, nrm, _ = mesh.filter_faces(m, self.last_visibility[0])
        if smooth is not None:
            (verts, faces, nrm, _), _ = mesh.smooth(mesh.Mesh(verts, faces, None, None), int(smooth), lo=lo32, scale=smooth_scale_of_grid(lo32, hi32),
                                                    normals=normals == "grid")  # (field normals are queried below)
        if simplify is not None:
            cell, dims = simplify_lattice_of_grid(grid_step(lo32, hi32, shape), shape, int(simplify))
            (verts, faces, nrm, _), _ = mesh.simplify(mesh.Mesh(verts, faces, None if normals == "field" else nrm, None), cell, lo32, dims)
        if normals == "field":
            nrm = field_normals(self.query_grad(verts)[2])
        if color and fused is not None:
            rgb, ok = mesh.tsdf_sample_color(fused, lo32, grid_step(lo32, hi32, shape), verts)
            miss = torch.nonzero(~ok).view(-1)  # (one host read of their number)
            self.last_fused_fallback = int(miss.numel())
            if miss.numel():
                rgb[miss] = self.query(verts[miss], -nrm[miss])[0]
        else:
            rgb = self.query(verts, -nrm)[0] if color else None
        m = mesh.Mesh(verts, faces, nrm, rgb)
        if texture is not None:
            shade = lambda p, d: self.query(p, d)[0]
            if fused is not None:
                def shade(p, d):
                    c, ok = mesh.tsdf_sample_color(fused, lo32, grid_step(lo32, hi32, shape), p)
                    return torch.where(ok[:, None], c, self.query(p, d)[0])
            F = int(faces.shape[0])
            self.last_texture = mesh.bake_texture(m, mesh.atlas_chart(F, int(texture)) if F else 2, shade)  # (no faces: an empty atlas)
        return m

    @torch.no_grad()
    def fuse_depth(self, views, lo, hi, res, trunc=None, depth="auto", min_opacity=0.5, carve=True, views_per_call=None, color=False,
                   depth_stat="mean", max_spread=None):
        """TSDF fusion of the model's own rendered depth: every camera of views = (poses_bound [n, 17], K_inv, H, W) is rendered with
        render(maps=True), its expected depth image is integrated into a truncated signed distance volume over the density grid's lattice
        of the box [lo, hi] at res (mesh.tsdf_integrate; rule T of include/nerf_hip.h), and the state (T, Wt) -- two fp32 [nx, ny, nz]
        device volumes -- is returned: mesh.tsdf_grid turns it into the array marching cubes takes at level 0.  The surface is then where
        the rendered views agree it is, not where sigma crosses a threshold; what the views see through is carved away.
        Per view and pixel with the maps (D, A): the depth is D / A where A >= min_opacity and +inf elsewhere, the opacity image is A; a
        pixel below min_opacity is background and, with carve, marks the lattice points along its ray as empty.  trunc: the truncation
        distance in world units; None = 4 x the largest lattice step (a choice, not a measurement).
        depth: "coarse" uses (D_c, A_c), "fine" (D_f, A_f), "auto" the fine pair under ``model.corrected`` and the coarse pair otherwise.
        In the default mode the fine pass sorts its five channels independently (quirk Q1), so D_f pairs weights
        with depths they do not belong to -- it is what compositing t like a colour gives --, while D_c is the physical expected depth of
        the coarse samples; with ``corrected`` the merged samples are sorted once and D_f is physical and sharper.
        depth_stat="mean" (default) fuses this EXPECTED depth: a ray that grazes a silhouette averages foreground and background, and a
        thin floater in front of a surface drags it forward.  depth_stat="median": the views are rendered with
        render(maps=True, quantiles=(0.25, 0.5, 0.75)) and the depth is Q(0.5) of the chosen pair (rule QD of include/nerf_hip.h) -- the
        depth in front of which half of the ray's weight lies, which stays on one of the two surfaces.  max_spread=s (world units, either
        statistic; None = off): a foreground pixel whose interquartile range Q(0.75) - Q(0.25) exceeds s gets depth NaN and so, by rule T,
        observes nothing and carves nothing -- rays whose weight is smeared or bimodal are left out instead of averaged in;
        ``self.last_tsdf_rejected`` counts them (0 without max_spread).  "mean" with max_spread=None makes no quantile call.
        The views are rendered one at a time (each a render() call of H * W rays: ``bf16_mlp`` / ``split_mlp`` apply as in render) and
        integrated views_per_call at a time (default: the kernel's views per launch), so no more than views_per_call depth and opacity
        images exist at once; the result does not depend on views_per_call.
        color=False: as above, and nothing more is allocated.  color=True: each view's C_fine of the same render(maps=True) call -- the
        image the view shows, whichever depth pair is chosen -- is kept as well (at most views_per_call colour images at once) and
        fused beside the depth (mesh.tsdf_integrate(rgb=, color=); rule TC of include/nerf_hip.h); the return is (T, Wt, C) with C
        mesh.tsdf_color_volume's fp32 [nx, ny, nz, 4]: the mean colour the views show within trunc of their surface, and the count."""
        import numpy as np

        from . import mesh

        if depth not in ("auto", "coarse", "fine"):
            raise ValueError(f"depth={depth!r}: 'auto', 'coarse' or 'fine'")
        if depth_stat not in ("mean", "median"):
            raise ValueError(f"depth_stat={depth_stat!r}: 'mean' or 'median'")
        if max_spread is not None and not float(max_spread) >= 0.0:
            raise ValueError(f"max_spread={max_spread!r}: None or a number >= 0 (world units)")
        quant = (0.25, 0.5, 0.75) if (depth_stat == "median" or max_spread is not None) else None
        self.last_tsdf_rejected = 0
        rejected = None
        col0 = 2 if depth == "fine" or (depth == "auto" and getattr(self, "corrected", False)) else 0
        per_call = _abi.TSDF_VIEWS_PER_LAUNCH if views_per_call is None else int(views_per_call)
        if per_call < 1:
            raise ValueError(f"views_per_call={views_per_call!r}: None or an int >= 1")
        ps = self._device_params()
        dev = ps[0].device
        poses_bound, K_inv, H, W = views
        H, W = int(H), int(W)
        pb = torch.as_tensor(poses_bound).reshape(-1, 17)
        shape = grid_shape(res)
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        step = grid_step(lo32, hi32, shape)
        T, Wt = mesh.tsdf_volume(shape, dev)
        C = mesh.tsdf_color_volume(shape, dev) if color else None
        n = int(pb.shape[0])
        if n == 0:
            return (T, Wt, C) if color else (T, Wt)
        row = torch.arange(H, device=dev).repeat_interleave(W)
        col = torch.arange(W, device=dev).repeat(H)
        inf = torch.full((), float("inf"), device=dev)
        D = torch.empty(min(per_call, n), H, W, device=dev)
        A = torch.empty_like(D)
        RGB = torch.empty(min(per_call, n), H, W, 3, device=dev) if color else None
        for v0 in range(0, n, per_call):
            k = min(per_call, n - v0)
            for c in range(k):
                out = self.render(row, col, pb[v0 + c].to(dev).expand(H * W, 17), K_inv, maps=True, quantiles=quant)
                M = out[2]
                d, a = M[:, col0], M[:, col0 + 1]
                if quant is None:
                    D[c] = torch.where(a >= min_opacity, d / a, inf).view(H, W)
                else:
                    dq, rej = tsdf_depth_image(d / a, a, out[3][:, col0 // 2], depth_stat, min_opacity, max_spread)
                    D[c] = dq.view(H, W)
                    rejected = rej.sum() if rejected is None else rejected + rej.sum()
                A[c] = a.view(H, W)
                if color:
                    RGB[c] = out[1].view(H, W, 3)
            kw = dict(rgb=RGB[:k], color=C) if color else {}
            mesh.tsdf_integrate(T, Wt, lo32, step, D[:k], pb[v0:v0 + k], K_inv, opacity=A[:k], trunc=trunc, min_opacity=min_opacity, carve=carve,
                                **kw)
        if rejected is not None:
            self.last_tsdf_rejected = int(rejected)
        return (T, Wt, C) if color else (T, Wt)

    @torch.no_grad()
    def extract_mesh_tsdf(self, views, lo, hi, res, trunc=None, depth="auto", min_opacity=0.5, carve=True, unseen="solid", color=True,
                          normals="grid", min_faces=None, keep_largest=None, simplify=None, smooth=None, visible=None, views_per_call=None,
                          depth_stat="mean", max_spread=None, texture=None):
        """A triangle mesh of the surface the rendered views agree on: fuse_depth(views, lo, hi, res, ...) -> mesh.tsdf_grid(T, Wt, unseen)
        -> mesh.marching_cubes at level 0 over the same lattice -> the stages of extract_mesh behind marching cubes, with the same keywords
        and order (min_faces / keep_largest, visible, smooth, simplify, then normals and colours at the final vertices).  No density
        threshold enters.  normals="grid": the TSDF lattice's normals (its central differences, pointing outward); "field" and the
        colours query the field at the final vertices as in extract_mesh.  unseen="solid" (default): lattice points no view observed count
        as inside, so the mesh closes behind what the cameras saw; with unseen="empty", or with carve=False, a second sheet appears one
        truncation distance behind the surface, where the observed band ends.  unseen="skip": marching cubes runs masked with
        valid = Wt > 0 (mesh.marching_cubes(valid=); rule M of include/nerf_hip.h) over the grid of "empty": triangles only from cells
        whose eight corners some view observed -- the surface the cameras saw and nothing else, open where they saw nothing.
        color=True: colours are queried from the field at the final vertices, seen along the inward normal; color=False: none.
        color="fused": the views' colours are fused with their depth (fuse_depth(color=True)) and sampled at the final vertices
        (mesh.tsdf_sample_color); only the vertices without a fused colour -- ``self.last_fused_fallback`` of them -- query the field.
        depth_stat / max_spread: fuse_depth's (the median depth instead of the mean; pixels whose interquartile depth range exceeds
        max_spread are left out; ``self.last_tsdf_rejected`` counts them).
        The state of the fusion is kept as ``self.last_tsdf`` = (T, Wt), or (T, Wt, C) with color="fused".
        texture=S: extract_mesh's -- ``self.last_texture``, baked for the final mesh; with color="fused" a texel takes the fused colour
        at its point (mesh.tsdf_sample_color) and the field's only where the volume has none, like the vertices."""
        import numpy as np

        from . import mesh

        _check_mesh_stages(normals, simplify, smooth)
        if unseen not in ("solid", "empty", "skip"):
            raise ValueError(f"unseen={unseen!r}: 'solid', 'empty' or 'skip'")
        if not (color is True or color is False or color == "fused"):
            raise ValueError(f"color={color!r}: True, False or 'fused'")
        fuse_color = color == "fused"
        shape = grid_shape(res)
        lo32 = np.asarray(lo, dtype=np.float32).reshape(3)
        hi32 = np.asarray(hi, dtype=np.float32).reshape(3)
        self.last_tsdf = self.fuse_depth(views, lo32, hi32, shape, trunc=trunc, depth=depth, min_opacity=min_opacity, carve=carve,
                                         views_per_call=views_per_call, color=fuse_color, depth_stat=depth_stat, max_spread=max_spread)
        T, Wt = self.last_tsdf[:2]
        if unseen == "skip":
            verts, faces, nrm = mesh.marching_cubes(mesh.tsdf_grid(T, Wt, "empty"), 0.0, lo32, grid_step(lo32, hi32, shape), valid=Wt > 0)
        else:
            verts, faces, nrm = mesh.marching_cubes(mesh.tsdf_grid(T, Wt, unseen), 0.0, lo32, grid_step(lo32, hi32, shape))
        return self._mesh_stages(verts, faces, nrm, lo32, hi32, shape, bool(color), normals, min_faces, keep_largest, simplify, smooth, visible,
                                 fused=self.last_tsdf[2] if fuse_color else None, texture=texture)

    @torch.no_grad()
    def render(self, row, column, poses_bound, K_inv, lo: int = 0, hi: int | None = None, fuse_rays: int = 16384, maps: bool = False,
               quantiles=None, normals=False):
        """Inference over a LONG list of rays (a frame, a test set) -- rays [lo, hi) of it -- with the reference's batch semantics and few
        kernel calls: the list is the sequence of batches [g*batch_ray, (g+1)*batch_ray) the reference's display loop feeds to `forward`
        (nerf.py:503-520), every ray gets exactly the bits a per-batch `forward` gives it (`fuse_plan`: consecutive batches whose ray 0
        has the same near / far share a launch of up to `fuse_rays` rays), and a 400-ray batch size no longer means 400-ray launches
        (0.71 of the fp32 roof, a fifth of the chip for the bf16 kernels).  The tail batch is rendered too (the reference drops it,
        nerf.py:442), with its own ray 0.  The weights must not change during the call.  Returns (C_coarse, C_fine) [hi - lo, 3].
        maps=True: every call is a nerf_hip_forward_maps call (same colour bits) and the return is (C_coarse, C_fine, maps) with maps
        [hi - lo, 4] = each ray's (D_c, A_c, D_f, A_f): expected depth and accumulated opacity of the coarse and the fine composite.
        quantiles (with maps=True; None = the call above): 1 .. 4 floats strictly inside (0, 1), e.g. (0.25, 0.5, 0.75).  Every call is a
        nerf_hip_forward_quantiles call (same colour and maps bits) and the return is (C_coarse, C_fine, maps, Q) with Q [hi - lo, 2, nq]:
        row 0 the coarse pass's, row 1 the fine pass's quantile depths (rule QD of include/nerf_hip.h; Q(0.5) is the median depth, where half
        of the ray's weight lies in front).  Batch semantics and fusing are unchanged.
        normals (with maps=True; False = the calls above, bit for bit): True or "fine", "coarse" or "both".  Every call is a
        nerf_hip_forward_normals call (same colour and maps bits) and Nrm [hi - lo, 2, 3] is appended LAST to the return (behind Q when
        quantiles is given too): row 0 the coarse pass's, row 1 the fine pass's N = sum_i w_i n_i, the field's normals -grad sigma /
        |grad sigma| at the call's own sample points composited with the ray's own weights (rule NM of include/nerf_hip.h; world frame,
        not normalised, |N| <= A; `unit_normals` makes an image of it).  Rows not asked for are NaN.  The gradients are exact fp32 in
        every mode and run at the gradient query's 70 M points/s: an exact-fp32 400 x 400 frame takes 3.0x ("fine") / 3.7x ("both") the
        maps frame, a bf16 one 19x / 26x."""
        quantiles = _check_quantiles(quantiles, maps)
        passes = _check_normals(normals, maps)
        ps = self._params()
        dev = ps[0].device
        n, Bm = row.shape[0], self.batch_ray
        hi = n if hi is None else hi
        C_c = torch.empty(max(hi - lo, 0), 3, dtype=torch.float32, device=dev)
        C_f = torch.empty_like(C_c)
        M = torch.empty(max(hi - lo, 0), 4, dtype=torch.float32, device=dev) if maps else None
        Q = torch.empty(max(hi - lo, 0), 2, len(quantiles), dtype=torch.float32, device=dev) if quantiles is not None else None
        Nrm = torch.full((max(hi - lo, 0), 2, 3), float("nan"), dtype=torch.float32, device=dev) if passes else None
        if hi <= lo:
            return _render_result(C_c, C_f, M, Q, Nrm)
        starts = torch.arange(0, n, Bm)
        nf0 = poses_bound[starts.to(poses_bound.device)][:, 15:17].to(torch.float32).cpu().tolist()  # ONE host copy per call
        plan = fuse_plan(nf0, n, Bm, lo, hi, fuse_rays)
        prev_ray0, prev_cap = self.ray0_near_far, self._ws_capacity
        try:
            self._ws_capacity = True
            self._workspace(max(MIN_CALL_RAYS, max(e - s for s, e, _, _ in plan)), _call_flags(self, False))  # ONE workspace, sized for the longest call
            if passes:
                self._normals_workspace(max(MIN_CALL_RAYS, max(e - s for s, e, _, _ in plan)), dev)  # (and ONE side workspace)
            with self.frozen_weights():
                for s, e, near, far in plan:
                    self.ray0_near_far = (near, far)
                    r_, c_, p_ = row[s:e], column[s:e], poses_bound[s:e]
                    if e - s < MIN_CALL_RAYS:
                        # a 1-ray piece (n % batch_ray == 1 behind a batch with another near / far; an unaligned shard that starts on a
                        # batch's last ray): the library needs B >= 2 like the reference (nerf.py:208 .squeeze()), so the piece is
                        # launched with its last ray repeated and the copy cropped -- rays are independent and ray0_near_far is handed
                        # over explicitly, so the real ray's bits do not change
                        k = MIN_CALL_RAYS - (e - s)
                        r_, c_, p_ = (torch.cat((x, x[-1:].expand(k, *x.shape[1:]))) for x in (r_, c_, p_))
                    out = self._launch(ps, r_, c_, p_, K_inv, maps=maps, quantiles=quantiles, normals=passes)
                    C_c[s - lo:e - lo] = out[0][: e - s]
                    C_f[s - lo:e - lo] = out[1][: e - s]
                    if maps:
                        M[s - lo:e - lo] = out[2][: e - s]
                    if Q is not None:
                        Q[s - lo:e - lo] = out[3][: e - s]
                    if Nrm is not None:
                        Nrm[s - lo:e - lo] = out[-1][: e - s]
        finally:
            self.ray0_near_far, self._ws_capacity = prev_ray0, prev_cap
        if getattr(self, "bf16_mlp", False):
            self.read_status()  # a frame is not handed out on a poisoned weight image (raises on STATUS_PREP_TIMEOUT; one sync per frame)
        return _render_result(C_c, C_f, M, Q, Nrm)


def _render_result(C_c, C_f, M, Q, Nrm=None):
    if Nrm is not None:
        return (C_c, C_f, M, Nrm) if Q is None else (C_c, C_f, M, Q, Nrm)
    if Q is not None:
        return C_c, C_f, M, Q
    return (C_c, C_f) if M is None else (C_c, C_f, M)


_NORMAL_PASSES = {"coarse": 1, "fine": 2, "both": 3}


def _check_normals(normals, maps) -> int:
    """render's normals keyword -> the passes of nerf_hip_forward_normals (0 = none; bit 0 coarse, bit 1 fine); needs maps=True"""
    if normals is False or normals is None:
        return 0
    if normals is True:
        normals = "fine"
    if not isinstance(normals, str) or normals not in _NORMAL_PASSES:
        raise ValueError(f"normals={normals!r}: False, True (= 'fine'), 'fine', 'coarse' or 'both'")
    if not maps:
        raise ValueError("normals needs maps=True: the normal maps come with the maps call")
    return _NORMAL_PASSES[normals]


def unit_normals(Nrm_row, A, min_opacity=0.5):
    """An image of unit normals from one row of render(normals=)'s Nrm: Nrm_row [..., 3] (the coarse or the fine pass's N) and that pass's
    opacity A [...] (torch tensors or numpy arrays) -> N / |N| where A >= min_opacity and |N| > 0, (0, 0, 0) elsewhere (background, rays
    whose normals cancel, NaN rows)."""
    xp = torch if torch.is_tensor(Nrm_row) else __import__("numpy")
    length = xp.sqrt((Nrm_row * Nrm_row).sum(-1))
    ok = (A >= min_opacity) & (length > 0)
    one = xp.ones_like(length)
    return xp.where(ok[..., None], Nrm_row / xp.where(ok, length, one)[..., None], xp.zeros_like(Nrm_row))


def _check_quantiles(quantiles, maps):
    """render's quantiles keyword -> None or a tuple of 1 .. _abi.MAX_QUANTILES floats strictly inside (0, 1); needs maps=True"""
    if quantiles is None:
        return None
    if not maps:
        raise ValueError("quantiles needs maps=True: the quantile depths come with the maps call")
    q = tuple(float(x) for x in quantiles)
    if not 1 <= len(q) <= _abi.MAX_QUANTILES or not all(0.0 < x < 1.0 for x in q):
        raise ValueError(f"quantiles={quantiles!r}: 1 .. {_abi.MAX_QUANTILES} numbers strictly inside (0, 1)")
    return q


def tsdf_depth_image(mean, a, Q3, depth_stat="mean", min_opacity=0.5, max_spread=None):
    """fuse_depth's depth-image rule over flat arrays (torch tensors or numpy arrays of one shape): mean = D / A of the chosen pair, a = its
    opacity A, Q3 = its quantile depths (Q(0.25), Q(0.5), Q(0.75)) [..., 3] or None (depth_stat="mean" with max_spread=None).
    -> (depth, rejected): the depth is the mean or the median Q(0.5) where a >= min_opacity (foreground) and +inf elsewhere; with
    max_spread = s a foreground pixel whose interquartile range Q(0.75) - Q(0.25) > s gets NaN (by rule T it observes nothing and carves
    nothing); rejected marks those pixels."""
    if depth_stat not in ("mean", "median"):
        raise ValueError(f"depth_stat={depth_stat!r}: 'mean' or 'median'")
    xp = torch if torch.is_tensor(a) else __import__("numpy")
    fg = a >= min_opacity
    d = Q3[..., 1] if depth_stat == "median" else mean
    inf, nan = (xp.full_like(a, v) for v in (float("inf"), float("nan")))
    d = xp.where(fg, d, inf)
    if max_spread is None:
        return d, xp.zeros_like(fg)
    rejected = fg & ((Q3[..., 2] - Q3[..., 0]) > max_spread)
    return xp.where(rejected, nan, d), rejected


def _check_mesh_stages(normals, simplify, smooth):
    """The keywords extract_mesh and extract_mesh_tsdf share, checked before any device work."""
    if normals not in ("grid", "field"):
        raise ValueError(f"normals={normals!r}: 'grid' or 'field'")
    if simplify is not None and (int(simplify) != simplify or int(simplify) < 2):
        raise ValueError(f"simplify={simplify!r}: None or an int >= 2 (cells of that many lattice steps)")
    if smooth is not None and (int(smooth) != smooth or int(smooth) < 1):
        raise ValueError(f"smooth={smooth!r}: None or an int >= 1 (Taubin iterations)")


def grid_shape(res) -> tuple:
    """res = n or (nx, ny, nz) -> (nx, ny, nz) as ints."""
    shape = (int(res),) * 3 if isinstance(res, (int,)) or (hasattr(res, "ndim") and res.ndim == 0) else tuple(int(n) for n in res)
    if len(shape) != 3:
        raise ValueError(f"res {res!r}: an int or three ints")
    return shape


def grid_step(lo32, hi32, shape):
    """The lattice step of NeRFModel.density_grid in fp32: (hi - lo) / (n - 1), 0 where n == 1."""
    import numpy as np

    n1 = np.asarray([max(n - 1, 1) for n in shape], dtype=np.float32)
    step = (np.asarray(hi32, dtype=np.float32) - np.asarray(lo32, dtype=np.float32)) / n1
    return np.where(np.asarray(shape) > 1, step, np.float32(0.0)).astype(np.float32)


def simplify_lattice_of_grid(step, shape, k: int):
    """The cluster lattice of extract_mesh(simplify=k) over a density grid of ``shape`` points and fp32 ``step``: cells of k lattice
    steps -> (cell [3] fp32 = fp32(k * step), 1 along an axis of one point, dims [3] = max(1, ceil((n - 1) / k)))."""
    import numpy as np

    step = np.asarray(step, dtype=np.float32).reshape(3)
    cell = np.where(np.asarray(shape) > 1, (np.float32(k) * step).astype(np.float32), np.float32(1.0)).astype(np.float32)
    dims = [max(1, -(-(int(n) - 1) // int(k))) for n in shape]
    return cell, dims


def smooth_scale_of_grid(lo32, hi32):
    """The box scale of extract_mesh(smooth=n): mesh.pow2_at_least of the largest fp32 extent of the grid's box [lo, hi]."""
    import numpy as np

    from .mesh import pow2_at_least

    return pow2_at_least((np.asarray(hi32, dtype=np.float32) - np.asarray(lo32, dtype=np.float32)).astype(np.float32).max())


def fuse_plan(near_far0, n: int, batch: int, lo: int = 0, hi: int | None = None, fuse_rays: int = 16384):
    """Kernel calls that render rays [lo, hi) of an n-ray list with the reference's batch semantics.  The reference renders the list in
    batches [g*batch, (g+1)*batch) and its resampler takes the coarse spacing from ray 0 OF EACH BATCH (nerf.py:233, quirk Q6) -- the
    only cross-ray term of the path.  Consecutive batches whose ray 0 has the same (near, far) can therefore share one call that is
    handed that pair: same bits per ray, fewer and fuller launches.  near_far0: [ceil(n / batch)][2] (near, far) of every batch's ray 0
    (host floats).  Returns [(s, e, near, far)], s < e, each call inside one run of equal pairs and at most `fuse_rays` rays long
    (at least one batch), pieces on the batch grid wherever the range allows it."""
    hi = n if hi is None else hi
    per_call = max(batch, fuse_rays // batch * batch)
    plan = []
    s = lo
    while s < hi:
        g = s // batch
        nf = (float(near_far0[g][0]), float(near_far0[g][1]))
        e = min((g + 1) * batch, hi)
        while e < hi and e - s + batch <= per_call:  # take the next batch along if its ray 0 agrees
            g2 = e // batch
            if (float(near_far0[g2][0]), float(near_far0[g2][1])) != nf:
                break
            e = min((g2 + 1) * batch, hi)
        plan.append((s, e, nf[0], nf[1]))
        s = e
    return plan


class _RayLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, C_c, C_f, C_t):
        C_c, C_f, C_t = C_c.contiguous(), C_f.contiguous(), C_t.contiguous().to(C_c.device, torch.float32)
        B = C_c.shape[0]
        loss = torch.empty(1, dtype=torch.float32, device=C_c.device)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dCc = torch.empty_like(C_c) if need else None
        dCf = torch.empty_like(C_f) if need else None
        _abi.check(_abi.lib().nerf_hip_ray_loss(C_c.data_ptr(), C_f.data_ptr(), C_t.data_ptr(), B, loss.data_ptr(),
                                                dCc.data_ptr() if need else None, dCf.data_ptr() if need else None,
                                                torch.cuda.current_stream(C_c.device).cuda_stream))
        if need:
            ctx.save_for_backward(dCc, dCf)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dCc, dCf = ctx.saved_tensors
        return g * dCc, g * dCf, None


def __getattr__(name):  # `from nerf import NeRFRunner` (main.py:4) without a circular import at module load
    if name == "NeRFRunner":
        from .train import NeRFRunner

        return NeRFRunner
    raise AttributeError(name)
