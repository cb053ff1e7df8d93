"""Train-loop side of the hot path: the fused optimizer and a runner with the
reference's ``NeRFRunner`` surface (``/root/reference/nerf.py:353-530``) that keeps the device busy -- GPU-resident
ray sampler, fused Adam, no per-iteration host sync (the reference flushes TensorBoard, copies ``C_true`` to the host
and updates a preview image every iteration, nerf.py:478-483).
"""
from __future__ import annotations

import contextlib
import glob
import numbers
import os
import time

import torch

from . import _abi
from .data import DeviceRays, NeRFDataset
from .nerf import NeRFModel


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` semantics (nerf.py:425: betas (0.9, 0.999), eps 1e-7, no weight decay) for the 24 tensors of
    ``model.network`` in ONE kernel launch (``nerf_hip_adam_step``).  A ``torch.optim.Optimizer`` subclass, so the
    reference's ``LambdaLR`` / ``MultiStepLR`` schedulers drive ``param_groups[0]['lr']`` unchanged; ``state_dict`` uses
    Adam's keys (``step``, ``exp_avg``, ``exp_avg_sq``)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        ps = [p for g in self.param_groups for p in g["params"]]
        if len(self.param_groups) != 1 or len(ps) != 24:
            raise ValueError("FusedAdam expects one group holding the 24 tensors of NeRFModel.network.parameters()")
        n = sum(p.numel() for p in ps)
        self._m = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
        self._v = torch.zeros_like(self._m)
        o = 0
        for p in ps:
            st = self.state[p]
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = self._m[o:o + p.numel()].view_as(p)
            st["exp_avg_sq"] = self._v[o:o + p.numel()].view_as(p)
            o += p.numel()
        self._step = 0

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        ps = self.param_groups[0]["params"]
        o = 0
        for p in ps:  # re-alias the flat buffers
            st = self.state[p]
            self._m[o:o + p.numel()].view_as(p).copy_(st["exp_avg"])
            self._v[o:o + p.numel()].view_as(p).copy_(st["exp_avg_sq"])
            st["exp_avg"] = self._m[o:o + p.numel()].view_as(p)
            st["exp_avg_sq"] = self._v[o:o + p.numel()].view_as(p)
            o += p.numel()
        self._step = int(self.state[ps[0]]["step"])

    def flat_state(self) -> dict:
        """What a resume needs, flat (parameters() order): {"step", "exp_avg" [593,924], "exp_avg_sq" [593,924]} on the host."""
        return {"step": int(self._step), "exp_avg": self._m.detach().cpu().clone(), "exp_avg_sq": self._v.detach().cpu().clone()}

    def load_flat_state(self, st: dict) -> None:
        if st["exp_avg"].numel() != self._m.numel() or st["exp_avg_sq"].numel() != self._v.numel():
            raise ValueError("optimizer state of another architecture")
        self._m.copy_(st["exp_avg"].to(self._m.device))
        self._v.copy_(st["exp_avg_sq"].to(self._v.device))
        self._step = int(st["step"])
        for p in self.param_groups[0]["params"]:
            self.state[p]["step"] = torch.tensor(float(self._step))

    @torch.no_grad()
    def step(self, closure=None):
        g = self.param_groups[0]
        ps = g["params"]
        if any(p.grad is None for p in ps):
            raise RuntimeError("FusedAdam.step: every parameter needs a gradient")
        self._step += 1
        b1, b2 = g["betas"]
        dev = ps[0].device
        _abi.check(_abi.lib().nerf_hip_adam_step(_abi.ptr_array(ps), _abi.ptr_array([p.grad.contiguous() for p in ps]),
                                                 self._m.data_ptr(), self._v.data_ptr(), self._step, float(g["lr"]), float(b1),
                                                 float(b2), float(g["eps"]), torch.cuda.current_stream(dev).cuda_stream))
        for p in ps:
            self.state[p]["step"] = torch.tensor(float(self._step))
        # bucket mode (model.grad_bucket: p.grad ARE views of a parallel.GradBucket): the gradients are used up, the next backward may
        # overwrite them
        from .parallel import consume_buckets_of

        consume_buckets_of(ps)
        return None

    def zero_grad(self, set_to_none: bool = True):
        """``Optimizer.zero_grad`` + bucket mode: dropping the gradients also releases the bucket they live in."""
        from .parallel import consume_buckets_of

        consume_buckets_of(self.param_groups[0]["params"])
        super().zero_grad(set_to_none=set_to_none)


class _NullWriter:
    def add_scalar(self, *a, **k):
        pass

    def flush(self):
        pass


def mask_train_step(model, row, col, poses_bound, K_inv, C_true, alpha, weight):
    """One train step with the alpha-mask loss (not in the reference): ``forward(maps=True)``, ``loss = ray_loss + weight * mask_loss`` (both
    sums over the batch), ``loss.backward()`` -- the gradients land where the autograd path puts them (``p.grad``, or the views of
    ``model.grad_bucket``).  Returns ``(C_coarse, C_fine, loss)`` detached, as ``NeRFModel.train_step`` does."""
    C_c, C_f, M = model(row, col, poses_bound, K_inv, maps=True)
    loss = model.ray_loss(C_c, C_f, C_true) + weight * model.mask_loss(M, alpha)
    loss.backward()
    return C_c.detach(), C_f.detach(), loss.detach()


def regularized_train_step(model, row, col, poses_bound, K_inv, C_true, alpha=None, mask_weight=0.0, dist_weight=0.0):
    """One train step with the optional extra loss terms (not in the reference): ``loss = ray_loss + mask_weight * mask_loss + dist_weight *
    distortion_loss`` (all sums over the batch), ``loss.backward()``, gradients as in ``mask_train_step``.  dist_weight > 0 takes
    ``forward(maps=True, distortion=True)`` (nerf_hip_forward_distortion_train / nerf_hip_backward_distortion); with
    dist_weight == 0 the forward is ``forward(maps=True)`` and nothing new runs.  mask_weight > 0 needs the batch's ``alpha``; a term whose
    weight is 0 is left out of the sum.  Returns ``(C_coarse, C_fine, loss)`` detached."""
    if dist_weight > 0:
        C_c, C_f, M, D = model(row, col, poses_bound, K_inv, maps=True, distortion=True)
    else:
        C_c, C_f, M = model(row, col, poses_bound, K_inv, maps=True)
    loss = model.ray_loss(C_c, C_f, C_true)
    if mask_weight > 0:
        loss = loss + mask_weight * model.mask_loss(M, alpha)
    if dist_weight > 0:
        loss = loss + dist_weight * model.distortion_loss(D)
    loss.backward()
    return C_c.detach(), C_f.detach(), loss.detach()


def _writer():
    try:
        from torch.utils.tensorboard import SummaryWriter  # absent offline

        return SummaryWriter()
    except Exception:
        return _NullWriter()


def _view_list(views) -> list:
    """views: an index or an iterable of indices -> a non-empty list of ints."""
    if isinstance(views, numbers.Integral):
        views = [views]
    try:
        views = list(views)
    except TypeError:
        raise ValueError(f"views={views!r}: an index or a list of indices") from None
    if not views or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in views):
        raise ValueError(f"views={views!r}: a non-empty list of integer indices (None selects every view)")
    return [int(v) for v in views]


def _check_views(views, pic_num: int, mode: str) -> None:
    bad = [v for v in views if not 0 <= v < pic_num]
    if bad:
        raise ValueError(f"views {bad}: the {mode!r} split has views 0 .. {pic_num - 1}")


class NeRFRunner:
    """The reference's runner surface: same 17 constructor arguments (nerf.py:354-372), ``trainer(mode)`` (nerf.py:445)
    and ``display()`` (nerf.py:503).  ``mode`` defaults to "train" so the reference's ``main.py:55`` call works.
    Extra keyword-only arguments: ``datasets`` (dict mode -> dataset, to run without files), ``log_every`` (host sync
    period; the reference syncs every iteration), ``bf16_mlp`` (BASELINE.json cfg3: the MLP on bf16 MFMA, default off), ``split_mlp`` (rendering calls -- validation,
    ``display()`` -- on the split-fp32 inference kernels: same 1e-4 bar, 3x the rate; training forwards ignore it; default off), ``split_train`` (the TRAIN
    step in split-fp32 arithmetic -- forward, dX chain and weight-gradient products on bf16 MFMA with two-part operands: 2x the exact fp32 step, gradients
    inside the bands the exact path is held to; default off, ignored with ``bf16_mlp``),
    ``on_resample_fault`` ("raise" | "warn" | "ignore": what to do when ANY iteration since the last logging point met the reference's
    exit(0) condition of nerf.py:251-253 -- a training run that has died; the kernels record it in a sticky status word, the device path
    itself clamps the index and goes on.  Default "raise": the reference stops there too), ``distributed`` (None: data-parallel iff a
    launcher started more than one rank; True: also with one rank -- rehearsals; False: never), ``overlap_allreduce`` (None: the
    NERF_DP_OVERLAP environment variable, default off; True: reduce the early 83 % of the gradient bucket on a side stream beside the last
    weight-gradient products), ``eval_every`` (None: off; N: every N iterations the held-out ``val`` split is evaluated -- ``evaluate("val",
    eval_views, save=False)``, every rank taking part -- its PSNR / SSIM logged as ``psnr/val`` / ``ssim/val`` and printed by rank 0; training
    is bit-identical to a run without it), ``eval_views`` (the view indices of those evaluations; None: all).

    **Data-parallel training (BASELINE.json cfg3) and tile-sharded rendering (cfg5)**: under ``python -m torch.distributed.run
    --nproc-per-node N .../main.py`` every rank builds this runner on ``cuda:LOCAL_RANK`` (RANK / WORLD_SIZE / LOCAL_RANK are read from
    the environment before any GPU call), joins one RCCL group (backend "nccl"), starts from rank 0's weights and draws the SAME
    permutation from the same sampler seed; of every global ``batch_ray`` batch a rank gathers only its contiguous slice
    (``parallel.shard_bounds``; the global ray 0's near / far go to every rank: quirk Q6), runs forward + loss + backward with the
    gradients written straight into one flat bucket, SUM-all-reduces it (one collective behind the step; optionally the early 83 % beside
    the last weight-gradient products) where the reference has ``loss.backward(); optimizer.step()`` (nerf.py:473-474) and takes the identical fused-Adam step.  Rank 0
    alone logs and writes checkpoints; ``display()`` deals the frames' reference batches out over the ranks with no collective in the
    data path and gathers the pixels afterwards."""

    def __init__(self, gpu=0, img_dir="../nerf_synthetic/lego/", results_path="./results/", ckpt_path="./checkpoint/", low_res=1,
                 total_iter=100000, batch_ray=400, learning=1e-3, lr_gamma=0.1, lr_milestone=(10, 200), n_coarse=64, n_fine=128,
                 data_type="sync", step=100, decay_end=200000, sched="EXP", continue_=False, *, datasets=None, log_every=None,
                 seed=624, bf16_mlp=False, split_mlp=False, split_train=False, on_resample_fault="raise", distributed=None, overlap_allreduce=None,
                 eval_every=None, eval_views=None, mask_weight=0.0, dist_weight=0.0):
        from . import nerf as _nerf
        from . import parallel as par

        if eval_every is not None and (isinstance(eval_every, bool) or not isinstance(eval_every, int) or eval_every < 1):
            raise ValueError(f"eval_every={eval_every!r}: None or a positive number of iterations")
        self.eval_every = eval_every
        self.eval_views = _view_list(eval_views) if eval_views is not None else None
        mask_weight = float(mask_weight)
        if not mask_weight >= 0.0 or mask_weight == float("inf"):
            raise ValueError(f"mask_weight={mask_weight!r}: a finite weight >= 0")
        self.mask_weight = mask_weight
        dist_weight = float(dist_weight)
        if not dist_weight >= 0.0 or dist_weight == float("inf"):  # (refused before anything touches the GPU, like mask_weight)
            raise ValueError(f"dist_weight={dist_weight!r}: a finite weight >= 0")
        self.dist_weight = dist_weight
        if mask_weight > 0 and datasets is None and data_type == "llff":  # (refused before anything touches the GPU or a process group)
            raise ValueError(f"MASK_WEIGHT = {mask_weight} needs the per-pixel alpha of the training images; LLFF captures carry none")

        # ---- the launcher's environment first: nothing above this line has touched the GPU
        self.env = par.DistEnv.from_env()
        self.distributed = (self.env.world > 1) if distributed is None else bool(distributed)
        if not self.distributed:
            self.env = par.DistEnv()  # a stray RANK in the environment of a deliberately single-process run
        self.rank, self.world = self.env.rank, self.env.world
        if not torch.cuda.is_available():
            raise RuntimeError("NeRFRunner needs a ROCm device: the MI355X path has no CPU fallback")
        # one process per GPU: under a launcher the rank's device is LOCAL_RANK; the ini's GPU key is the single-process choice
        self.device = torch.device("cuda:" + str(self.env.local_rank if self.env.launched and self.distributed else gpu))
        _nerf.device = self.device  # module global like nerf.py:387
        torch.cuda.set_device(self.device)
        self.group = None
        if self.distributed:
            import torch.distributed as dist

            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", "29500")
                # "nccl" IS RCCL on ROCm (xGMI).  NERF_DIST_BACKEND=gloo: rehearsals with several ranks on ONE GPU (RCCL refuses two
                # ranks on one device); gloo moves device tensors through the host, same collectives, same results
                backend = os.environ.get("NERF_DIST_BACKEND", "nccl")
                kw_pg = {"device_id": self.device} if backend == "nccl" else {}
                dist.init_process_group(backend, rank=self.rank, world_size=self.world, **kw_pg)
        self.writer = _writer() if self.rank == 0 else _NullWriter()
        self.start_time = time.strftime("%m-%d-%H-%M-%S", time.localtime())
        if self.distributed:  # one name for the job's checkpoints / results: rank 0's clock
            import torch.distributed as dist

            box = [self.start_time]
            dist.broadcast_object_list(box, src=0)
            self.start_time = box[0]
        self.results_path, self.ckpt_path, self.low_res = results_path, ckpt_path, low_res
        self.total_iter, self.batch_ray, self.step, self.decay_end = total_iter, batch_ray, step, decay_end
        self.log_every = log_every or step
        if on_resample_fault not in ("warn", "raise", "ignore"):
            raise ValueError("on_resample_fault: 'warn', 'raise' or 'ignore'")
        self.on_resample_fault = on_resample_fault
        self.resample_fault_iter = None  # first logging point at which the reference's exit(0) condition had been met since the previous one
        # this rank's slice of every global batch: the model is built for the slice (its kernels see B = local rays)
        self.lo, self.hi = par.shard_bounds(batch_ray, self.rank, self.world)
        self.local_rays = self.hi - self.lo
        if self.local_rays < 2:
            raise ValueError(f"BATCH_RAY = {batch_ray} over {self.world} ranks leaves rank {self.rank} {self.local_rays} ray(s): the path needs >= 2 per rank")
        self.model = NeRFModel(num_coarse=n_coarse, num_fine=n_fine, batch_ray=self.local_rays).to(self.device)

        # resume: newest "<anything>_<iter>.pkl" (nerf.py:404-415); every rank reads the same file (one node, one filesystem)
        last_iter, last_ckpt = -1, None
        if continue_:
            for f in glob.glob(ckpt_path + "*.pkl"):
                it = int(f.split("_")[-1][:-4])
                if it > last_iter:
                    last_iter, last_ckpt = it, f
        if last_ckpt is not None:
            self.model = torch.load(last_ckpt, weights_only=False, map_location=self.device).to(self.device)
            self.model.batch_ray = self.local_rays  # (the checkpoint holds the CONFIGURED batch size; this rank's kernels see its slice)
        self.last_iter = last_iter
        self.model.bf16_mlp = bool(bf16_mlp)  # an attribute, not part of the checkpoint format: set after a resume too
        self.model.split_mlp = bool(split_mlp)
        self.model.split_train = bool(split_train)  # opt-in: the train step in split-fp32 arithmetic (2x the exact step's rate)
        # the gradients of every step live in ONE flat buffer whose views are p.grad (the kernels write straight into it: no 24 fresh
        # tensors per iteration) -- the all-reduce buffer of a data-parallel run
        self.bucket = par.GradBucket(self.model.network.parameters())
        if self.distributed:
            par.broadcast_parameters(self.model.network.parameters(), src=0)  # replicated weights, whatever each rank's RNG drew
            # The early 83 % of the bucket (point_layer[0..7]) can be reduced on a side stream beside the last weight-gradient products
            # (GradBucket.enable_overlap).  OPT-IN (overlap_allreduce=True or NERF_DP_OVERLAP=1): measured on a single-rank RCCL group the split
            # launches and the two cross-stream hand-offs cost 46-62 us per step (scripts/dp_step_proxy.py) -- what an 8-rank ring all-reduce
            # of these 2.27 MiB is priced at in the first place -- while ONE collective behind the step costs 1-6 us there.
            if overlap_allreduce if overlap_allreduce is not None else os.environ.get("NERF_DP_OVERLAP") == "1":
                self.bucket.enable_overlap()

        def ds(mode):
            if datasets is not None:
                return datasets[mode]
            return NeRFDataset(root_dir=img_dir, low_res=low_res, transform=None, type=data_type, mode=mode)

        self.train_dataset, self.val_dataset, self.disp_dataset = ds("train"), ds("val"), ds("test")
        if self.mask_weight > 0 and getattr(self.train_dataset, "all_alpha", None) is None:
            raise ValueError(f"MASK_WEIGHT = {self.mask_weight} needs the per-pixel alpha of the training images; this dataset has none "
                             f"(data_type={data_type!r}: LLFF captures carry no alpha)")
        # the SAME seeds on every rank: the ranks draw identical permutations and take disjoint slices of every batch
        self.train_rays = DeviceRays(self.train_dataset, self.device, seed)
        self.val_rays = DeviceRays(self.val_dataset, self.device, seed + 1)
        self.disp_rays = DeviceRays(self.disp_dataset, self.device, seed + 2)
        self.height, self.width, self.focal = self.train_dataset.height, self.train_dataset.width, self.train_dataset.focal
        self.num_pic = self.train_dataset.pic_num
        if self.eval_views is not None and self.eval_every is not None:
            _check_views(self.eval_views, self.val_rays.pic_num, "val")
        self._eval_ws = {}  # the model's inference workspaces while it is evaluated (_evaluation)
        # inverse intrinsics, transposed (nerf.py:433)
        self.K_inv = torch.tensor([[1.0, 0.0, -0.5 * self.width], [0.0, -1.0, 0.5 * self.height], [0.0, 0.0, -self.focal]]).to(torch.float).transpose(0, 1)

        self.optimizer = FusedAdam([{"params": list(self.model.network.parameters()), "initial_lr": learning}], lr=learning,
                                   betas=(0.9, 0.999), eps=1e-7)
        # resume: "<time>_<iter>.opt" beside the checkpoint (written by this runner; absent for a reference-written checkpoint) restores
        # Adam's moments / step and the sampler's position, so that N iterations == k + resume + (N - k) bit for bit in fp32
        self._resume_sampler = None
        if last_ckpt is not None:
            st = self._load_opt_state(last_ckpt)
            if st is not None:
                self._resume_sampler = (st.get("mode", "train"), st["sampler"])
        if sched == "EXP":  # nerf.py:426, including its post-decay_end multiplier lr_gamma * learning
            self.scheduler = torch.optim.lr_scheduler.LambdaLR(
                self.optimizer, lr_lambda=lambda it: lr_gamma ** (it / decay_end) if it < decay_end else lr_gamma * learning,
                last_epoch=self.last_iter)
        else:
            self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, list(lr_milestone), lr_gamma, last_epoch=self.last_iter)

    # ----- the two collectives of the logging point (data-parallel runs only; every rank reaches them at the same iterations) -----
    def _global_loss_and_fault(self, loss, fault: bool, error: bool = False):
        """-> (global loss, any rank's resample fault, any rank's error).  ONE SUM and ONE MAX collective; a rank-local error (a raised
        NerfHipError at the logging point) travels as a flag through the MAX so that EVERY rank raises afterwards -- a rank that left the
        loop alone would leave the others blocked in the next all_reduce until the RCCL timeout."""
        lv = float(loss.detach())
        if not self.distributed:
            return lv, fault, error
        import torch.distributed as dist

        from . import parallel as par

        total = par.allreduce_host_scalars([lv], dist.ReduceOp.SUM, self.device, self.group)[0]  # the loss is a SUM over rays (nerf.py:328-331)
        flags = par.allreduce_host_scalars([1.0 if fault else 0.0, 1.0 if error else 0.0], dist.ReduceOp.MAX, self.device, self.group)
        return total, flags[0] > 0.0, flags[1] > 0.0  # the same decisions on every rank

    # ----- checkpoints: the reference's whole-module pickle (nerf.py:491) + what a bit-exact resume needs beside it -----
    def _save_checkpoint(self, it: int, rays, mode: str, epoch_gen_state, next_batch: int):
        os.makedirs(self.ckpt_path, exist_ok=True)
        stem = self.ckpt_path + self.start_time + "_" + str(it)
        # the module is pickled with the CONFIGURED batch size: a data-parallel rank's model is built for its slice (e.g. 512 of 4096), but
        # the checkpoint must load anywhere and equal a single-process checkpoint of the same config (nerf.py:491, reloaded at :415)
        prev = self.model.batch_ray
        self.model.batch_ray = self.batch_ray
        try:
            torch.save(self.model, stem + ".pkl")
        finally:
            self.model.batch_ray = prev
        # "<time>_<iter>.opt": Adam's moments and step (flat, parameters() order) and the sampler's position -- the reference saves neither
        # (a resumed reference run restarts Adam from zero moments and its DataLoader from a fresh shuffle); absent file = that behaviour
        torch.save({"format": 1, "iter": it, "mode": mode, "adam": self.optimizer.flat_state(),
                    "sampler": {"epoch_gen_state": epoch_gen_state.cpu(), "next_batch": int(next_batch)}}, stem + ".opt")

    def _load_opt_state(self, ckpt: str):
        path = ckpt[:-4] + ".opt"
        if not os.path.exists(path):
            return None
        st = torch.load(path, weights_only=False, map_location="cpu")
        self.optimizer.load_flat_state(st["adam"])
        return st

    # nerf.py:445-499
    def trainer(self, mode="train"):
        from . import parallel as par

        rays = {"train": self.train_rays, "val": self.val_rays, "disp": self.disp_rays}[mode]
        it = self.last_iter + 1
        t0, n0 = time.perf_counter(), it
        t_eval = 0.0  # seconds spent in evaluations (eval_every), left out of the printed rate
        self.model.train()
        skip = 0
        if self._resume_sampler is not None and self._resume_sampler[0] == mode:
            # continue the interrupted epoch: the generator state its permutation was drawn from, and the batches already used
            rays.gen.set_state(self._resume_sampler[1]["epoch_gen_state"].cpu())
            skip = int(self._resume_sampler[1]["next_batch"])
        self._resume_sampler = None
        while it < self.total_iter:
            epoch_gen_state = rays.gen.get_state()  # (a host copy of the generator's 16 bytes of Philox state: no device sync)
            masked = self.mask_weight > 0  # the alpha of every batch's pixels rides behind `pic`
            batches = (rays.epoch_sharded(self.batch_ray, self.rank, self.world, first_batch=skip, with_alpha=masked) if self.distributed
                       else rays.epoch(self.batch_ray, first_batch=skip, with_alpha=masked))
            bi = skip - 1
            skip = 0
            for batch in batches:
                bi += 1
                row, col, pix_val, poses_bound, pic = batch[:5]
                # (no zero_grad: the backward kernels OVERWRITE the bucket's views, which ARE p.grad; FusedAdam.step releases the bucket)
                if self.distributed:
                    # this rank's slice of the batch: forward + loss + backward into the flat bucket, ONE SUM all-reduce (nerf.py:473-474)
                    _, _, loss = par.train_step_local(self.model, self.bucket, row, col, poses_bound, self.K_inv, pix_val, batch[-1],
                                                      self.world, self.group, alpha=batch[5] if masked else None,
                                                      mask_weight=self.mask_weight, dist_weight=self.dist_weight)
                elif self.dist_weight > 0:
                    # ... + DIST_WEIGHT * distortion_loss through autograd (forward(maps=True, distortion=True), nerf_hip_backward_distortion)
                    self.model.grad_bucket = self.bucket
                    try:
                        _, _, loss = regularized_train_step(self.model, row, col, poses_bound, self.K_inv, pix_val, batch[5] if masked else None,
                                                            self.mask_weight, self.dist_weight)
                    finally:
                        self.model.grad_bucket = None
                elif masked:
                    # ray_loss + MASK_WEIGHT * mask_loss through autograd (forward(maps=True), nerf_hip_backward_maps) into the bucket
                    self.model.grad_bucket = self.bucket
                    try:
                        _, _, loss = mask_train_step(self.model, row, col, poses_bound, self.K_inv, pix_val, batch[5], self.mask_weight)
                    finally:
                        self.model.grad_bucket = None
                else:
                    # nerf.py:470-473 (forward, ray_loss, backward) as ONE library call: same kernels, no interpreter between them
                    self.model.grad_bucket = self.bucket
                    try:
                        _, _, loss = self.model.train_step(row, col, poses_bound, self.K_inv, pix_val)
                    finally:
                        self.model.grad_bucket = None
                self.optimizer.step()
                self.scheduler.step()
                if (it + 1) % self.log_every == 0:  # the only host sync of the loop
                    # the reference checks its resampling indices in EVERY forward and exit(0)s when a ray's coarse weights have all
                    # vanished (nerf.py:251-253) -- the state a run that has died stays in.  The kernels keep the bit in a sticky word
                    # across iterations; it is looked at here, where the loop syncs anyway, so nothing between two logs is missed
                    err = None
                    try:
                        fault = self.on_resample_fault != "ignore" and self.model.resample_fault_since(clear=True)
                    except _abi.NerfHipError as e:  # rank-local (e.g. STATUS_PREP_TIMEOUT): raised on EVERY rank behind the collectives below
                        err, fault = e, False
                    lv, fault, any_err = self._global_loss_and_fault(loss, fault, err is not None)
                    if any_err:
                        raise err if err is not None else _abi.NerfHipError(f"iteration <= {it}: another rank reported a library error at this logging point")
                    dt = time.perf_counter() - t0 - t_eval
                    self.writer.add_scalar("loss/" + mode, lv, it)
                    self.writer.add_scalar("lr/" + mode, self.optimizer.param_groups[0]["lr"], it)
                    self.writer.flush()
                    if self.rank == 0:
                        print(f"[ITER] {it} [LOSS] {lv:.4f} [LR] {self.optimizer.param_groups[0]['lr']:.3e} "
                              f"[{(it + 1 - n0) * self.batch_ray / max(dt, 1e-9):,.0f} rays/s" + (f", {self.world} ranks]" if self.distributed else "]"))
                    if fault:
                        if self.resample_fault_iter is None:
                            self.resample_fault_iter = it
                            if self.rank == 0:
                                print(f"[ITER] {it} resample index out of range since the last log: the reference prints its banner and exit(0)s "
                                      "there (nerf.py:251-253); this path clamps the index" +
                                      (" and trains on (on_resample_fault='warn')" if self.on_resample_fault == "warn" else ""))
                        if self.on_resample_fault == "raise":
                            from .nerf import ResampleIndexError

                            raise ResampleIndexError(f"iteration <= {it}: resample index outside [0, Nf-1] (the reference exit(0)s here, nerf.py:251-253); "
                                                     "NeRFRunner(on_resample_fault='warn') trains on")
                if (it + 1) % self.step == 0 and self.rank == 0:
                    self._save_checkpoint(it, rays, mode, epoch_gen_state, bi + 1)
                if self.eval_every is not None and (it + 1) % self.eval_every == 0:
                    # every rank renders its share of the views; nothing the loop reads changes (_evaluation)
                    r = self._evaluate("val", self.eval_views, False, it)
                    if r is not None:
                        t_eval += r["seconds"]
                        self.writer.add_scalar("psnr/val", r["psnr"], it)
                        self.writer.add_scalar("ssim/val", r["ssim"], it)
                        self.writer.flush()
                        print(f"[EVAL] {it} [PSNR] {r['psnr']:.3f} dB [SSIM] {r['ssim']:.4f} [{len(r['views'])} val views, {r['seconds']:.2f} s]")
                it += 1
                if it >= self.total_iter:
                    break
            if mode == "val":
                break
        self.last_iter = it - 1
        return self.last_iter

    # ----- held-out evaluation (not in the reference, which only writes the frames: nerf.py:503-530) -----
    def _split_rays(self, mode: str):
        splits = {"train": self.train_rays, "val": self.val_rays, "disp": self.disp_rays}
        if mode not in splits:
            raise ValueError(f"mode={mode!r}: 'train', 'val' or 'disp'")
        return splits[mode]

    @contextlib.contextmanager
    def _evaluation(self):
        """Rendering for an evaluation without touching what the training loop reads: the model's inference calls run on workspaces of
        their own (so a ray that meets the resample condition leaves no bit in the sticky status words ``resample_fault_since`` reads at
        the logging points), on the reference's batch grid, and the model's train / eval mode comes back as it was (it is pickled into
        the checkpoints)."""
        m = self.model
        saved = (m._ws, m._last_ws, m.batch_ray, m.training)
        m._ws, m.batch_ray = self._eval_ws, self.batch_ray
        m.eval()
        try:
            yield m
        finally:
            self._eval_ws = m._ws
            m._ws, m._last_ws, m.batch_ray = saved[:3]
            m.train(saved[3])

    def render_view(self, i: int, mode: str = "disp"):
        """View i of a split ("train", "val" or "disp") rendered as its own ray list: its pixels in row-major order through
        NeRFModel.render on the ``batch_ray`` grid, every pixel including the tail batch, with the model's inference flags.  Where the
        split's views share near / far these are display()'s bits wherever display() renders the pixel.  Under a launcher every rank
        must call it: the view's reference batches are dealt out as in display() (render_rows_sharded + gather_rows) and every rank gets
        the whole frame.  Returns (frame, gt), [H, W, 3] fp32 device tensors."""
        from . import parallel as par

        rays = self._split_rays(mode)
        (i,) = _view_list(i)
        _check_views([i], rays.pic_num, mode)
        H, W = rays.height, rays.width
        n = H * W
        row, col, pix, poses_bound, _ = rays.gather(torch.arange(i * n, (i + 1) * n, device=self.device))
        with torch.no_grad(), self._evaluation() as m:
            if self.distributed:
                r = par.render_rows_sharded(m, row, col, poses_bound, self.K_inv, self.rank, self.world)
                C = par.gather_rows(r[2].to(self.device), n, self.rank, self.world, self.group, batch=self.batch_ray)
            else:
                C = m.render(row, col, poses_bound, self.K_inv)[1]
        return C.reshape(H, W, 3), pix.reshape(H, W, 3)

    def evaluate(self, mode="disp", views=None, save=True):
        """Held-out metrics of the current model on a split ("disp": the "test" dataset display() renders, "val", "train"): every selected
        view (``views``: indices, None = all) is rendered by render_view() and scored against its ground truth by ``nerf_hip_image_metrics``
        (metrics.py: MSE, PSNR = -10 log10 MSE with data range 1, SSIM with an 11-tap Gaussian window, valid filtering).  Under a launcher
        every rank must call it; the metrics are computed on rank 0 and the other ranks return None.  Returns {"iter", "mode", "views",
        "psnr", "ssim", "mse", "per_view": [{"view", "psnr", "ssim", "mse"}], "seconds"}, the means over views (PSNR averaged per view, as
        papers report it); with save, rank 0 writes it to ``<results_path><start_time>_<last_iter>_eval.json``."""
        return self._evaluate(mode, views, save, self.last_iter)

    def _evaluate(self, mode, views, save, it):
        import json

        import numpy as np

        from . import ops
        from .metrics import psnr_from_mse

        rays = self._split_rays(mode)
        views = list(range(rays.pic_num)) if views is None else _view_list(views)
        _check_views(views, rays.pic_num, mode)
        t0 = time.perf_counter()
        mses, ssims = [], []
        for i in views:
            frame, gt = self.render_view(i, mode)
            if self.rank == 0:
                mse, ssim = ops.image_metrics(frame[None], gt[None])
                mses.append(mse)
                ssims.append(ssim)
        if self.rank != 0:
            return None
        mse, ssim = torch.cat(mses).cpu().numpy(), torch.cat(ssims).cpu().numpy()  # (the one host sync)
        psnr = psnr_from_mse(mse)
        out = {"iter": int(it), "mode": mode, "views": views, "psnr": float(np.mean(psnr)), "ssim": float(np.mean(ssim)),
               "mse": float(np.mean(mse)),
               "per_view": [{"view": v, "psnr": float(p), "ssim": float(s), "mse": float(e)} for v, p, s, e in zip(views, psnr, ssim, mse)],
               "seconds": time.perf_counter() - t0}
        if save:
            path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_eval.json"
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
        return out

    def density_grid(self, res, lo=(-1.5,) * 3, hi=(1.5,) * 3, save=True):
        """sigma of the current model on a res^3 (or res = (nx, ny, nz)) lattice spanning the box [lo, hi] (NeRFModel.density_grid: exact
        fp32, lattice point (i, j, k) = lo + (i, j, k) * step, step = (hi - lo) / (n - 1)).  save: writes
        ``<results_path><start_time>_<last_iter>_sigma<res>.npz`` with ``sigma`` (float32 [nx, ny, nz]), ``lo``, ``hi``, ``step`` and ``iter``
        -- the input of a marching-cubes mesh extraction.  Under a launcher only rank 0 computes and writes the grid; the
        other ranks return None.  Returns sigma as a numpy array."""
        import numpy as np

        from .nerf import grid_shape, grid_step

        if self.rank != 0:
            return None
        shape = grid_shape(res)
        lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
        self.model.eval()
        sigma = self.model.density_grid(lo32, hi32, shape).cpu().numpy()
        if save:
            tag = str(shape[0]) if len(set(shape)) == 1 else "x".join(str(n) for n in shape)
            path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_sigma" + tag + ".npz"
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            np.savez(path, sigma=sigma, lo=lo32, hi=hi32, step=grid_step(lo32, hi32, shape), iter=np.int64(self.last_iter))
        return sigma

    def bake_volume(self, res, lo=(-1.5,) * 3, hi=(1.5,) * 3, degree=2, sigma_min=0.0, block=8, save=True, preview=None, finetune=0,
                    finetune_batch=4096, finetune_lr=None, finetune_tv=None, finetune_upsample=(), finetune_prune=None, compact=None,
                    finetune_compact=False, vq=None, vq_iters=10, vq_prune=None, vq_keep=0.0, vq_finetune=0, vq_finetune_batch=4096,
                    vq_lr_sigma=None, vq_lr_coef=None):
        """The current model baked into an SH radiance volume on a res^3 (or res = (nx, ny, nz)) lattice over the box [lo, hi]
        (NeRFModel.bake_volume: exact fp32; volume.py) -> the volume.Volume.  save: writes it with volume.save to
        ``<results_path><start_time>_<last_iter>_volume<res>.npz``.  preview: None, or "train" / "val" / "test" -- every view of that
        split is rendered FROM THE VOLUME (volume.render_views: no network) and, with save, written to ``<i>_volume.png`` beside the
        display frames; the frames are scored against NeRFModel.render of the same views (metrics.image_metrics) and one ``[VOLUME]``
        line prints the mean PSNR / SSIM.  Under a launcher only rank 0 bakes, renders and writes, without any collective (the comparison
        frames are rendered whole on rank 0, not through render_view's sharded path); the other ranks return None at once.
        finetune > 0: the baked volume is then fine-tuned for that many Adam steps of finetune_batch rays against the TRAIN split's own
        pixels with the support frozen (volume.finetune; finetune_lr: None, (lr_sigma, lr_coef) or Finetuner's keywords), on rank 0 as
        the bake; the fine-tuned volume is returned and, with save, also written to ``..._volume<res>_ft<finetune>.npz``; one more
        ``[VOLUME] ... finetune`` line prints the first and the last batch loss and, with preview, the split's PSNR / SSIM against its
        GROUND-TRUTH images before and after.  finetune = 0 computes, prints and writes nothing new.
        COARSE TO FINE (volume.finetune): finetune_tv = None or (tv_sigma, tv_coef), the total-variation weights; finetune_upsample =
        the step counts after which the lattice is doubled (k of them give a (2^k (res - 1) + 1)^3 volume, written as
        ``..._ft<finetune>_up<k>.npz``); finetune_prune = None, or the density at or below which a point is cleared before each
        doubling.  The finetune line then names the final lattice and the TV weights; without these arguments nothing changes.
        COMPACT (volume.CompactVolume, rule VC): compact = "fp32" / "fp16" bakes straight into the rows of the active points
        (NeRFModel.bake_volume(compact=)), returns that form, names the file ``..._volume<res>_c32.npz`` / ``_c16.npz``, renders the
        preview from the compact form, and the first ``[VOLUME]`` line gains the compact and the dense byte counts.  With finetune > 0
        the bake and the fine-tuning stay dense and each volume is packed before it is written, previewed or returned.  compact = None
        computes, prints and writes nothing new.
        finetune_compact = True (needs compact and finetune > 0: ValueError) trains the compact form itself: the bake goes straight into
        fp32 rows, the dense coefficient array is never allocated, the fine-tuning is volume.finetune_compact, and each volume is
        converted to ``compact``'s element type when it is written, previewed or returned.  The files hold the same arrays and carry
        the same names; the finetune line gains the word ``compact``.
        VECTOR QUANTISATION (volume.quantize): vq = K (needs compact: ValueError) scores every row of the
        volume that is returned -- after any fine-tuning -- by the rendering weight the TRAIN split's views give it
        (volume.importance_views), quantises it with a K-code codebook (vq_iters k-means iterations, vq_prune / vq_keep the
        importance shares that are dropped / kept verbatim) and, with save, writes the VQVolume beside the compact file as
        ``<the compact file's stem>_vq<K>.npz``.  One ``[VOLUME] ... vq`` line prints the class counts and the byte counts; with
        preview the split is also rendered from the DEQUANTIZED volume and both PSNR / SSIM pairs against the ground-truth images are
        printed.  The return value stays the compact volume; self.last_volume_vq holds the numbers and the path.  vq = None computes,
        prints and writes nothing new.
        VQ FINE-TUNING (volume.finetune_vq): vq_finetune = ITERS > 0 (needs vq: ValueError) then trains the
        VQVolume's codebook, kept rows and sigma for ITERS Adam steps of vq_finetune_batch rays (at most 2^20) against the TRAIN
        split's own pixels, the codes frozen (vq_lr_sigma / vq_lr_coef: None, or VQFinetuner's rates), and, with save, writes the tuned
        VQVolume beside the untuned file as ``<...>_vq<K>_ft<ITERS>.npz``.  The vq line and self.last_volume_vq gain the first and the
        last batch loss (first_loss, last_loss, finetune_iters, finetune_seconds, finetune_path) and, with preview, the tuned PSNR /
        SSIM (psnr_vq_ft, ssim_vq_ft).  vq_finetune = 0 computes, prints and writes nothing new."""
        import numpy as np

        from . import volume
        from .mesh import png_bytes
        from .metrics import image_metrics
        from .nerf import grid_shape

        if preview is not None and preview not in ("train", "val", "test"):
            raise ValueError(f"preview={preview!r}: None, 'train', 'val' or 'test'")
        if int(finetune) != finetune or finetune < 0:
            raise ValueError(f"finetune={finetune!r}: a number of steps >= 0")
        if compact not in (None, "fp32", "fp16"):
            raise ValueError(f"compact={compact!r}: None, 'fp32' or 'fp16'")
        if finetune_compact and (compact is None or not finetune):
            raise ValueError("finetune_compact trains the compact form: it needs compact = 'fp32' / 'fp16' and finetune > 0")
        if vq is not None:
            if compact is None:
                raise ValueError("vq quantises the compact form: it needs compact = 'fp32' / 'fp16'")
            from .volume import _check_k, _share
            vq, vq_iters = _check_k(vq, vq_iters)
            _share(vq_keep, "vq_keep"), (None if vq_prune is None else _share(vq_prune, "vq_prune"))
        if isinstance(vq_finetune, bool) or int(vq_finetune) != vq_finetune or vq_finetune < 0:
            raise ValueError(f"vq_finetune={vq_finetune!r}: a number of steps >= 0")
        if vq_finetune and vq is None:
            raise ValueError("vq_finetune trains the quantised form: it needs vq = K")
        if vq_finetune and not 1 <= int(vq_finetune_batch) <= volume.VQ_MAX_RAYS:
            raise ValueError(f"vq_finetune_batch={vq_finetune_batch!r}: 1 .. 2^20 rays per step")
        ctag = "" if compact is None else {"fp32": "_c32", "fp16": "_c16"}[compact]
        shape = grid_shape(res)
        tv = (0.0, 0.0) if finetune_tv is None else tuple(float(w) for w in finetune_tv)
        if len(tv) != 2:
            raise ValueError(f"finetune_tv={finetune_tv!r}: None or (tv_sigma, tv_coef)")
        if not finetune and (tuple(finetune_upsample) or finetune_prune is not None or any(tv)):
            raise ValueError("finetune_tv / finetune_upsample / finetune_prune need finetune > 0")
        if finetune:
            volume._check_tv(tv[0], tv[1], 1e-9)
            ups, _ = volume.check_schedule(shape, finetune, finetune_upsample, finetune_prune)
        if self.rank != 0:
            return None
        self.model.eval()
        t0 = time.perf_counter()
        vol = self.model.bake_volume(np.asarray(lo, np.float32), np.asarray(hi, np.float32), shape, degree=degree, sigma_min=sigma_min,
                                     block=block, compact="fp32" if finetune_compact else (None if finetune else compact))
        if finetune_compact:
            vol, rows32 = volume.convert(vol, compact), vol  # written and previewed as asked for; fine-tuned on fp32 rows
        elif compact is not None and finetune:
            vol, dense = volume.pack(vol, compact), vol      # written and previewed compact; fine-tuned dense
        torch.cuda.synchronize(self.device)
        if compact is None:
            active = int((vol.coef[..., 0, :] != 0).any(dim=-1).sum())
            print(f"[VOLUME] {self.last_iter} {'x'.join(str(n) for n in shape)} degree {degree}: {active} / {vol.sigma.numel()} lattice points "
                  f"hold colour, {int(vol.occ.sum())} / {vol.occ.numel()} blocks of {vol.block} occupied, "
                  f"{(vol.sigma.numel() * 4 + vol.coef.numel() * 4) / 2**20:.1f} MiB, {time.perf_counter() - t0:.2f} s")
        else:
            npts = int(np.prod(shape))
            active = int((vol.coef[:, :3] != 0).any(dim=-1).sum())
            print(f"[VOLUME] {self.last_iter} {'x'.join(str(n) for n in shape)} degree {degree}: {active} / {npts} lattice points "
                  f"hold colour, {int(vol.occ.sum())} / {vol.occ.numel()} blocks of {vol.block} occupied, {int(vol.sigma.shape[0])} rows, "
                  f"compact {compact} {volume.nbytes(vol)} bytes (dense {npts * (4 + 12 * (int(degree) + 1) ** 2) + vol.occ.numel()} bytes), "
                  f"{time.perf_counter() - t0:.2f} s")
        if save:
            tag = str(shape[0]) if len(set(shape)) == 1 else "x".join(str(n) for n in shape)
            path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_volume" + tag + ctag + ".npz"
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            volume.save(path, vol)
        if preview is not None:
            rays = {"train": self.train_rays, "val": self.val_rays, "test": self.disp_rays}[preview]
            H, W = rays.height, rays.width
            n = H * W
            psnr, ssim = [], []
            for i in range(rays.pic_num):
                frame = volume.render_views(vol, rays.poses[i:i + 1], self.K_inv, H, W)[0][0]
                # the model's own frame on THIS rank alone (no collective: the other ranks have returned), as the mesh paths render
                row, col, _, poses_bound, _ = rays.gather(torch.arange(i * n, (i + 1) * n, device=self.device))
                with torch.no_grad(), self._evaluation() as mdl:
                    exact = mdl.render(row, col, poses_bound, self.K_inv)[1].reshape(H, W, 3)
                m = image_metrics(frame[None], exact[None])
                psnr.append(float(m["psnr"][0]))
                ssim.append(float(m["ssim"][0]))
                if save:
                    save_dir = self.results_path + self.start_time + "/"
                    os.makedirs(save_dir, exist_ok=True)
                    with open(save_dir + str(i) + "_volume.png", "wb") as f:
                        f.write(png_bytes(np.rint(frame.clamp(0, 1).cpu().numpy() * 255.0).astype(np.uint8)))
            print(f"[VOLUME] {self.last_iter} {preview} preview vs model.render [PSNR] {np.mean(psnr):.3f} dB [SSIM] {np.mean(ssim):.4f} "
                  f"[{rays.pic_num} views]")
            self.last_volume_preview = {"psnr": float(np.mean(psnr)), "ssim": float(np.mean(ssim)), "views": rays.pic_num}
        if finetune:
            def against_truth(v):
                rays = {"train": self.train_rays, "val": self.val_rays, "test": self.disp_rays}[preview]
                H, W = rays.height, rays.width
                truth = rays.pixels.view(rays.pic_num, H, W, 3)
                ms = [image_metrics(volume.render_views(v, rays.poses[i:i + 1], self.K_inv, H, W)[0], truth[i:i + 1]) for i in range(rays.pic_num)]
                return float(np.mean([float(m["psnr"][0]) for m in ms])), float(np.mean([float(m["ssim"][0]) for m in ms]))

            lrs = {} if finetune_lr is None else (dict(finetune_lr) if isinstance(finetune_lr, dict) else
                                                  dict(zip(("lr_sigma", "lr_coef"), finetune_lr)))
            before = against_truth(vol) if preview is not None else None
            t0 = time.perf_counter()
            if any(tv):
                lrs.update(tv_sigma=tv[0], tv_coef=tv[1])
            if finetune_compact:
                vol = None                                   # the converted copy of the bake is not kept through the training
                vol, losses = volume.finetune_compact(rows32, self.train_rays, self.K_inv, int(finetune), batch=int(finetune_batch),
                                                      upsample_at=ups, prune=finetune_prune, **lrs)
                rows32 = None
            else:
                vol, losses = volume.finetune(vol if compact is None else dense, self.train_rays, self.K_inv, int(finetune), batch=int(finetune_batch), upsample_at=ups,
                                              prune=finetune_prune, **lrs)
            losses = losses.cpu().numpy()
            seconds = time.perf_counter() - t0
            final_shape = tuple(int(n) for n in (vol.shape if finetune_compact else vol.sigma.shape))
            if finetune_compact:
                vol = volume.convert(vol, compact)
            elif compact is not None:
                dense = None
                vol = volume.pack(vol, compact)
            self.last_volume_finetune = {"iters": int(finetune), "first_loss": float(losses[0]), "last_loss": float(losses[-1]), "seconds": seconds,
                                         "shape": final_shape}
            scores = ""
            if preview is not None:
                after = against_truth(vol)
                scores = (f", {preview} views vs ground truth [PSNR] {before[0]:.3f} -> {after[0]:.3f} dB [SSIM] {before[1]:.4f} -> "
                          f"{after[1]:.4f}")
                self.last_volume_finetune.update(psnr_before=before[0], psnr_after=after[0], ssim_before=before[1], ssim_after=after[1])
            extra = ""
            if ups:
                extra += f", {len(ups)} upsample{'s' if len(ups) > 1 else ''} to {'x'.join(str(n) for n in final_shape)}"
                if finetune_prune is not None:
                    extra += f" pruned at {float(finetune_prune):g}"
            if any(tv):
                extra += f", TV sigma {tv[0]:g} coef {tv[1]:g}"
            print(f"[VOLUME] {self.last_iter} finetune{' compact' if finetune_compact else ''} {int(finetune)} steps of {int(finetune_batch)} train rays{extra}: batch loss "
                  f"{losses[0]:.3e} -> {losses[-1]:.3e}{scores}, {seconds:.2f} s")
            if save:
                tag = str(shape[0]) if len(set(shape)) == 1 else "x".join(str(n) for n in shape)
                up = f"_up{len(ups)}" if ups else ""
                volume.save(self.results_path + self.start_time + "_" + str(self.last_iter) + "_volume" + tag + "_ft" + str(int(finetune)) + up +
                            ctag + ".npz", vol)
        if vq is not None:
            t0 = time.perf_counter()
            tr = self.train_rays
            imp, _ = volume.importance_views(vol, tr.poses[:tr.pic_num], self.K_inv, tr.height, tr.width, views_per_call=4)
            vqv = volume.quantize(vol, imp, K=vq, iters=vq_iters, prune_share=vq_prune, keep_share=vq_keep)
            counts = [int((vqv.cls == k).sum()) for k in (0, 1, 2)]
            seconds = time.perf_counter() - t0
            self.last_volume_vq = {"K": int(vqv.codebook.shape[0]), "pruned": counts[0], "coded": counts[1], "kept": counts[2],
                                   "nbytes": volume.nbytes(vqv), "compact_nbytes": volume.nbytes(vol), "seconds": seconds, "path": None}
            scores = ""
            if preview is not None:
                rays = {"train": self.train_rays, "val": self.val_rays, "test": self.disp_rays}[preview]
                H, W = rays.height, rays.width
                truth = rays.pixels.view(rays.pic_num, H, W, 3)

                def truth_scores(v):
                    ms = [image_metrics(volume.render_views(v, rays.poses[i:i + 1], self.K_inv, H, W)[0], truth[i:i + 1]) for i in range(rays.pic_num)]
                    return float(np.mean([float(m["psnr"][0]) for m in ms])), float(np.mean([float(m["ssim"][0]) for m in ms]))

                was, now = truth_scores(vol), truth_scores(volume.dequantize(vqv))
                scores = (f", {preview} views vs ground truth [PSNR] compact {was[0]:.3f} dB dequantized {now[0]:.3f} dB [SSIM] compact "
                          f"{was[1]:.4f} dequantized {now[1]:.4f}")
                self.last_volume_vq.update(psnr_compact=was[0], psnr_vq=now[0], ssim_compact=was[1], ssim_vq=now[1])
            tuned = None
            if vq_finetune:
                t1 = time.perf_counter()
                vq_lrs = {k: float(x) for k, x in (("lr_sigma", vq_lr_sigma), ("lr_coef", vq_lr_coef)) if x is not None}
                tuned, vq_losses = volume.finetune_vq(vqv, tr, self.K_inv, int(vq_finetune), batch=int(vq_finetune_batch), **vq_lrs)
                vq_losses = vq_losses.cpu().numpy()
                self.last_volume_vq.update(finetune_iters=int(vq_finetune), first_loss=float(vq_losses[0]), last_loss=float(vq_losses[-1]),
                                           finetune_seconds=time.perf_counter() - t1, finetune_path=None)
                scores += (f", vq finetune {int(vq_finetune)} steps of {int(vq_finetune_batch)} train rays: batch loss {vq_losses[0]:.3e} -> "
                           f"{vq_losses[-1]:.3e}")
                if preview is not None:
                    ft = truth_scores(volume.dequantize(tuned))
                    scores += f" [PSNR] tuned {ft[0]:.3f} dB [SSIM] tuned {ft[1]:.4f}"
                    self.last_volume_vq.update(psnr_vq_ft=ft[0], ssim_vq_ft=ft[1])
            print(f"[VOLUME] {self.last_iter} vq {self.last_volume_vq['K']} codes, {vq_iters} iterations over {tr.pic_num} train views: "
                  f"{counts[0]} rows pruned, {counts[1]} coded, {counts[2]} kept, {volume.nbytes(vqv)} bytes (compact {volume.nbytes(vol)} bytes)"
                  f"{scores}, {seconds:.2f} s")
            if save:
                tag = str(shape[0]) if len(set(shape)) == 1 else "x".join(str(n) for n in shape)
                ft = ("_ft" + str(int(finetune)) + (f"_up{len(ups)}" if ups else "")) if finetune else ""
                path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_volume" + tag + ft + ctag + f"_vq{vq}.npz"
                if os.path.dirname(path):
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                volume.save(path, vqv)
                self.last_volume_vq["path"] = path
                if tuned is not None:
                    volume.save(path[:-4] + f"_ft{int(vq_finetune)}.npz", tuned)
                    self.last_volume_vq["finetune_path"] = path[:-4] + f"_ft{int(vq_finetune)}.npz"
        return vol

    def extract_mesh(self, res, level, lo=(-1.5,) * 3, hi=(1.5,) * 3, color=True, save=True, normals="grid", band=None, min_faces=None,
                     keep_largest=None, simplify=None, smooth=None, compare=None, compare_samples=200_000, compare_tau=(), visible_from=None,
                     tsdf_from=None, tsdf_trunc=None, tsdf_every=1, tsdf_color=False, tsdf_unseen="solid", tsdf_depth_stat="mean",
                     tsdf_max_spread=None, texture=None):
        """A triangle mesh of the current model's isosurface sigma == level over a res^3 (or res = (nx, ny, nz)) lattice spanning [lo, hi]
        (NeRFModel.extract_mesh: the density grid's lattice, marching cubes on the device, vertex colours seen along the inward
        normals).  save: writes ``<results_path><start_time>_<last_iter>_mesh<res>.ply`` (binary PLY, mesh.write_ply: positions,
        normals and, with color, uchar colours).  Under a launcher only rank 0 computes and writes the mesh; the other ranks return
        None.  Returns mesh.Mesh of numpy arrays (rgb None without color).  normals: "grid" (marching-cubes normals from the grid) or
        "field" (the field's analytic gradient at each vertex), as NeRFModel.extract_mesh.  band: None (the dense grid) or a block size
        r >= 2 -- the field is evaluated only in a band of r^3-point blocks around the surface (NeRFModel.density_band: far fewer points,
        the same mesh wherever the band finds the surface; a component smaller than a block can be missed).  min_faces / keep_largest: drop
        the floaters on the device before normals and colours are queried -- keep the connected components with at least min_faces faces
        and, with keep_largest=k, among the k with the most faces (NeRFModel.extract_mesh; both None: no filtering).  With band= the band
        may already have missed islands smaller than a block, and filtering removes the rest.  simplify: None or an int k >= 2 -- the mesh
        is simplified on the device by vertex clustering in cells of k lattice steps, after the filter and before normals and colours
        are queried (NeRFModel.extract_mesh).  smooth: None or an int n >= 1 -- n Taubin smoothing iterations on the device after the
        filter and before simplify (NeRFModel.extract_mesh, mesh.smooth).  Same file name either way.  compare: None, or a
        ground-truth mesh -- the path of a PLY file (mesh.read_ply) or a mesh.Mesh -- against which the extracted mesh is measured on the
        device after it is written: mesh.compare(extracted, ground truth, n=compare_samples, thresholds=compare_tau) -- Chamfer
        distance, precision / recall / F-score per threshold, both meshes' area and volume.  The result is kept as
        ``self.last_mesh_eval``, printed on one line and, with save, written to ``<results_path><start_time>_<last_iter>_mesh_eval.json``.
        Without compare nothing new is computed, printed or written.  visible_from: None, or "train" / "val" / "test" -- the faces that
        no camera of that split sees go before smoothing, simplification, normals and colours (NeRFModel.extract_mesh(visible=): one
        shadow ray per face and camera on the device); one ``[MESH]`` line says how many faces were seen.  Same file name either way;
        without it nothing new is computed, printed or written.  tsdf_from: None, or "train" / "val" / "test" -- the mesh is not the
        isosurface of sigma but the zero set of a TSDF volume fused from the model's rendered depth of every tsdf_every-th camera of
        that split over the same lattice (NeRFModel.extract_mesh_tsdf: truncation distance tsdf_trunc, None = 4 lattice steps; unseen
        space solid, background rays carve).  ``level`` and ``band`` are then ignored -- the ``[MESH] ... [TSDF]`` line says so, with
        the views, the lattice points observed and the truncation distance -- and the file name gets ``_tsdf`` before ``.ply``.  Without
        it nothing new is computed, printed or written.  tsdf_color=True (with tsdf_from and color): the vertex colours are fused from
        the same rendered views (NeRFModel.extract_mesh_tsdf(color="fused")); tsdf_unseen: "solid" (default), "empty" or "skip" -- "skip"
        meshes only what the cameras observed (masked marching cubes).  With either, the ``[TSDF]`` line also counts the lattice points
        with a fused colour and the vertices that fell back to the field, and the file name gets ``_fused`` and / or ``_skip`` after
        ``_tsdf``.  Without them the line and the name are unchanged.  tsdf_depth_stat: "mean" (default) or "median" -- the views' median
        depth Q(0.5) is fused instead of their expected depth (NeRFModel.fuse_depth(depth_stat=): it stays on one surface where a ray
        grazes a silhouette or passes a thin floater); tsdf_max_spread: None, or a distance s >= 0 in world units -- pixels whose
        interquartile depth range exceeds s are left out of the fusion (fuse_depth(max_spread=)).  With either, the ``[TSDF]`` line also
        names the statistic and counts the rejected pixels, and "median" puts ``_median`` right after ``_tsdf`` in the file name.
        texture: None, or an int S (with color) -- a texture atlas of at most S x S texels is baked for the final mesh
        (NeRFModel.extract_mesh(texture=): the field, or with tsdf_color the fused volume, at every texel; kept as
        ``self.model.last_texture``); one ``[MESH] ... [TEXTURE]`` line gives the atlas's size, the chart, the faces and the share of
        owned texels, and with save the mesh is also written as ``<...>_mesh<res>.obj`` / ``.mtl`` / ``.png`` beside the ``.ply``
        (mesh.write_obj).  The returned Mesh and the ``.ply`` are unchanged; without it nothing new is computed, printed or written."""
        import numpy as np

        from .mesh import Mesh, write_obj, write_ply
        from .mesh import tsdf_trunc as default_trunc
        from .nerf import grid_shape, grid_step

        if self.rank != 0:
            return None
        shape = grid_shape(res)
        lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
        self.model.eval()
        kw = {}
        if visible_from is not None:
            if visible_from not in ("train", "val", "test"):
                raise ValueError(f"visible_from={visible_from!r}: None, 'train', 'val' or 'test'")
            rays = {"train": self.train_rays, "val": self.val_rays, "test": self.disp_rays}[visible_from]
            kw["visible"] = (rays.poses, self.K_inv, rays.height, rays.width)
        if texture is not None:
            kw["texture"] = int(texture)
        if tsdf_from is not None:
            if tsdf_from not in ("train", "val", "test"):
                raise ValueError(f"tsdf_from={tsdf_from!r}: None, 'train', 'val' or 'test'")
            if int(tsdf_every) != tsdf_every or int(tsdf_every) < 1:
                raise ValueError(f"tsdf_every={tsdf_every!r}: an int >= 1")
            if tsdf_unseen not in ("solid", "empty", "skip"):
                raise ValueError(f"tsdf_unseen={tsdf_unseen!r}: 'solid', 'empty' or 'skip'")
            fused = bool(tsdf_color) and bool(color)
            extended = bool(tsdf_color) or tsdf_unseen != "solid"
            if extended:
                kw["unseen"] = tsdf_unseen
            if tsdf_depth_stat not in ("mean", "median"):
                raise ValueError(f"tsdf_depth_stat={tsdf_depth_stat!r}: 'mean' or 'median'")
            quant = tsdf_depth_stat != "mean" or tsdf_max_spread is not None
            if quant:
                kw["depth_stat"], kw["max_spread"] = tsdf_depth_stat, tsdf_max_spread
            rays = {"train": self.train_rays, "val": self.val_rays, "test": self.disp_rays}[tsdf_from]
            poses = rays.poses[::int(tsdf_every)]
            m = self.model.extract_mesh_tsdf((poses, self.K_inv, rays.height, rays.width), lo32, hi32, shape, trunc=tsdf_trunc,
                                             color="fused" if fused else color, normals=normals, min_faces=min_faces,
                                             keep_largest=keep_largest, simplify=simplify, smooth=smooth,
                                             **kw)
            Wt = self.model.last_tsdf[1]
            trunc = default_trunc(grid_step(lo32, hi32, shape)) if tsdf_trunc is None else float(tsdf_trunc)
            more = ""
            if extended:
                coloured = int((self.model.last_tsdf[2][..., 3] > 0).sum()) if fused else 0
                by_field = self.model.last_fused_fallback if fused else (len(m.verts) if color else 0)
                more = f", {coloured} lattice points with a colour, {by_field} vertices coloured by the field"
            if quant:
                spread = "" if tsdf_max_spread is None else f" (depth spread > {float(tsdf_max_spread):.6g})"
                more += f", {tsdf_depth_stat} depth, {self.model.last_tsdf_rejected} pixels rejected{spread}"
            print(f"[MESH] {self.last_iter} [TSDF] {len(poses)} {tsdf_from} views fused, {int((Wt > 0).sum())} / {Wt.numel()} lattice points "
                  f"observed, trunc {trunc:.6g}{more} (level {level!r} ignored: the surface is the fused depth's)")
        else:
            m = self.model.extract_mesh(lo32, hi32, shape, level, color=color, normals=normals, band=band, min_faces=min_faces,
                                        keep_largest=keep_largest, simplify=simplify, smooth=smooth, **kw)
        if visible_from is not None:
            seen, per_cam = self.model.last_visibility
            print(f"[MESH] {self.last_iter} [VISIBLE] {int(seen.sum())} / {int(seen.numel())} faces seen from the {len(per_cam)} {visible_from} "
                  f"cameras (per camera {min(per_cam, default=0)} .. {max(per_cam, default=0)})")
        out = Mesh(*(None if a is None else a.cpu().numpy() for a in m))
        if texture is not None:
            tex = self.model.last_texture
            th, tw = (int(n) for n in tex.mask.shape)
            print(f"[MESH] {self.last_iter} [TEXTURE] {tw} x {th}, chart {tex.chart}, {tex.faces} faces, "
                  f"{int(tex.mask.sum()) / max(th * tw, 1):.3f} of the texels owned")
        if save:
            tag = str(shape[0]) if len(set(shape)) == 1 else "x".join(str(n) for n in shape)
            tsdf_tag = "" if tsdf_from is None else "_tsdf" + ("_median" if tsdf_depth_stat == "median" else "") + ("_fused" if fused else "") + ("_skip" if tsdf_unseen == "skip" else "")
            path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_mesh" + tag + tsdf_tag + ".ply"
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            write_ply(path, out.verts, out.faces, out.normals, out.rgb)
            if texture is not None:
                write_obj(path[:-4] + ".obj", out, tex)
        if compare is not None:
            self.last_mesh_eval = self._compare_mesh(m, compare, compare_samples, compare_tau, save)
        return out

    def _compare_mesh(self, m, truth, samples, taus, save):
        """extract_mesh(compare=): mesh.compare of the device mesh m against truth (a PLY path or a Mesh) -> the result as plain
        Python numbers; printed, and with save written beside the mesh."""
        import json

        import numpy as np

        from . import mesh as M

        name = None
        if not isinstance(truth, M.Mesh):
            name = os.fspath(truth)
            tv, tf, _, _ = M.read_ply(name)
            truth = M.Mesh(tv, tf, None, None)
        dev = m.verts.device
        truth = M.Mesh(torch.as_tensor(np.asarray(truth.verts, np.float32) if not torch.is_tensor(truth.verts) else truth.verts).to(dev),
                       torch.as_tensor(np.asarray(truth.faces, np.int32) if not torch.is_tensor(truth.faces) else truth.faces).to(dev), None, None)
        r = M.compare(M.Mesh(m.verts, m.faces, None, None), truth, n=int(samples), thresholds=tuple(taus))
        for k in ("measure_a", "measure_b"):
            ms = r[k]
            r[k] = dict(area=ms.area, volume=ms.volume, centroid=[float(c) for c in ms.centroid], faces=ms.faces)
        r.update(iter=int(self.last_iter), truth=name)
        per_tau = " ".join(f"[F@{t:g}] {f:.4f} (P {p:.4f} R {q:.4f})" for t, f, p, q in zip(r["thresholds"], r["fscore"], r["precision"], r["recall"]))
        print(f"[MESH-EVAL] {r['iter']} [CHAMFER] {r['chamfer']:.6g} (mesh->truth {r['a_to_b']['mean']:.6g}, truth->mesh {r['b_to_a']['mean']:.6g}) "
              f"{per_tau + ' ' if per_tau else ''}[AREA] {r['measure_a']['area']:.6g} vs {r['measure_b']['area']:.6g} [VOLUME] "
              f"{r['measure_a']['volume']:.6g} vs {r['measure_b']['volume']:.6g} [{r['samples']} samples, clamped {r['clamped']}]")
        if save:
            path = self.results_path + self.start_time + "_" + str(self.last_iter) + "_mesh_eval.json"
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                json.dump(r, fh, indent=1)
        return r

    # nerf.py:503-530
    def display(self, save=True, maps=False, normals=False):
        """Renders every display frame (white where the reference's loop leaves a pixel out) and returns them, [pic, H, W, 3] numpy.
        maps=True: also the fine expected depth and accumulated opacity of every rendered pixel (NeRFModel.render(maps=True): D_f, A_f;
        NaN depth and 0 opacity where the frame stays white), returned as (frames, depth, acc) with depth / acc [pic, H, W] fp32; with save,
        rank 0 also writes ``<results_path><start_time>_<last_iter>_maps.npz`` (``depth``, ``acc``, and every frame's ``near`` / ``far``)
        and ``<i>_depth.png`` (depth normalised by the frame's near / far) and ``<i>_acc.png`` previews beside the frames.
        normals=True (with maps=True): also the fine pass's composited field normal N_f of every rendered pixel
        (NeRFModel.render(normals="fine"), rule NM of include/nerf_hip.h; world frame, not normalised, 0 where the frame stays white),
        returned as (frames, depth, acc, normal) with normal [pic, H, W, 3] fp32; with save, rank 0 also writes ``<i>_normal.png`` beside
        the frames: 0.5 + 0.5 * nerf.unit_normals(normal, acc), so the background is mid grey."""
        if normals and not maps:
            raise ValueError("normals needs maps=True: the normal maps come with the maps call")
        rays = self.disp_rays
        result = torch.full((rays.pic_num, self.height, self.width, 3), 1.0, device=self.device)
        if maps:
            depth = torch.full((rays.pic_num, self.height, self.width), float("nan"), device=self.device)
            acc = torch.zeros((rays.pic_num, self.height, self.width), device=self.device)
        if normals:
            nrm = torch.zeros((rays.pic_num, self.height, self.width, 3), device=self.device)
        self.model.eval()
        # the reference's loop (batches of batch_ray rays in pixel order, the tail < batch stays white) through NeRFModel.render: batches
        # whose ray 0 has the same near / far share kernel calls -- same bits per pixel, launches of up to 16,384 rays instead of 400
        n_keep = rays.num_pix // self.batch_ray * self.batch_ray
        chunk = max(1, (1 << 20) // self.batch_ray) * self.batch_ray  # rays gathered per step (on the batch grid)
        from . import parallel as par

        prev_batch = self.model.batch_ray
        self.model.batch_ray = self.batch_ray  # the grid of the reference's display batches (a data-parallel rank's model is built for its slice)
        try:
            with torch.no_grad():
                for s in range(0, n_keep, chunk):
                    row, col, pix_val, poses_bound, pic = rays.gather(torch.arange(s, min(s + chunk, n_keep), device=self.device))
                    if self.distributed:
                        # cfg5: the chunk's reference batches dealt out over the ranks (shards on the batch grid, every call handed its
                        # batches' ray 0: same pixels for any world size), NO collective in the data path; the picture is assembled after
                        r = par.render_rows_sharded(self.model, row, col, poses_bound, self.K_inv, self.rank, self.world, maps=maps, normals=normals)
                        C_fine = par.gather_rows(r[2].to(self.device), row.shape[0], self.rank, self.world, self.group, batch=self.batch_ray)
                        M = par.gather_rows(r[3].to(self.device), row.shape[0], self.rank, self.world, self.group, batch=self.batch_ray) if maps else None
                        Nf = par.gather_rows(r[4].to(self.device), row.shape[0], self.rank, self.world, self.group, batch=self.batch_ray) if normals else None
                    else:
                        r = self.model.render(row, col, poses_bound, self.K_inv, maps=maps, normals="fine" if normals else False)
                        C_fine, M = r[1], (r[2] if maps else None)
                        Nf = r[-1][:, 1] if normals else None
                    result[pic, row, col] = C_fine
                    if normals:
                        nrm[pic, row, col] = Nf
                    if maps:
                        depth[pic, row, col] = M[:, 2]
                        acc[pic, row, col] = M[:, 3]
        finally:
            self.model.batch_ray = prev_batch
        result = result.cpu().numpy()
        if save and self.rank == 0:
            save_dir = self.results_path + self.start_time + "/"
            os.makedirs(save_dir, exist_ok=True)
            try:
                import matplotlib.pyplot as plt

                for i in range(rays.pic_num):
                    plt.imsave(save_dir + str(i) + ".jpg", result[i].clip(0, 1))
            except Exception as e:  # pragma: no cover
                print("display: could not write images:", e)
            try:
                import imageio
                import numpy as np

                imageio.mimwrite(self.results_path + self.start_time + "_" + str(self.last_iter) + ".mp4",
                                 (result * 255.0).astype(np.uint8), fps=30)
            except Exception:
                pass  # imageio is optional (absent offline)
        if not maps:
            return result
        depth, acc = depth.cpu().numpy(), acc.cpu().numpy()
        if save and self.rank == 0:
            import numpy as np

            nf = rays.poses[:, 15:17].cpu().numpy()  # every frame's near / far as the kernels see them
            np.savez(self.results_path + self.start_time + "_" + str(self.last_iter) + "_maps.npz", depth=depth, acc=acc,
                     near=nf[:, 0].copy(), far=nf[:, 1].copy())
            try:
                import matplotlib.pyplot as plt

                for i in range(rays.pic_num):
                    d = (depth[i] - nf[i, 0]) / (nf[i, 1] - nf[i, 0])
                    plt.imsave(save_dir + str(i) + "_depth.png", np.nan_to_num(d, nan=1.0).clip(0, 1), cmap="gray", vmin=0.0, vmax=1.0)
                    plt.imsave(save_dir + str(i) + "_acc.png", acc[i].clip(0, 1), cmap="gray", vmin=0.0, vmax=1.0)
            except Exception as e:  # pragma: no cover
                print("display: could not write map previews:", e)
        if not normals:
            return result, depth, acc
        nrm = nrm.cpu().numpy()
        if save and self.rank == 0:
            import numpy as np

            from .mesh import png_bytes
            from .nerf import unit_normals

            for i in range(rays.pic_num):
                img = 0.5 + 0.5 * unit_normals(nrm[i], acc[i])
                with open(save_dir + str(i) + "_normal.png", "wb") as f:
                    f.write(png_bytes(np.rint(img.clip(0, 1) * 255.0).astype(np.uint8)))
        return result, depth, acc, nrm
