#!/usr/bin/env python3
"""bench.py -- rays/s of the MI355X volume-rendering hot path on BASELINE.json's cfg2 workload.

A "step" = one full forward of the hot path (ray generation, 64 coarse + 128 fine samples per ray,
encode, 8x256 MLP per sample, resample, merge/sort, composite) over one batch of 4096 synthetic rays of
a 400x400 lego-like view, fp32, inputs already resident in HBM.  That is the headline `value`.  A plain run does only what
that figure needs: set-up, W warm-up and K timed steps, the --dump-outputs arrays if asked for, the result line.  With --full
the same run also times the other configurations of the path (fp32 train step, bf16-MLP forward and train step: BASELINE.json
cfg3; the split-fp32 forms) for a fraction of a second each, reports them under `extra`, each with its own roofline block, and
adds everything marked --full below.

Contract (driver):  python bench.py --gpus N --steps K --warmup W
  * N > 1 and no RANK in the environment: this process only LAUNCHES -- before torch.cuda or the HIP library is touched it
    starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
    as a child, relays rank 0's single JSON line and exits with the child's code (never exec: MI355X pool rule).
  * N > 1 under a launcher (RANK / WORLD_SIZE set): one rank per GPU over RCCL.  Every rank renders its own 4096-ray
    batches -- image-space ray batches are independent units, so the data path has no collective: scaling = "weak".
    The train legs add the one real exchange of the path, a SUM all-reduce of the 593,924 fp32 gradients (2.27 MiB) in one
    flat bucket the backward kernels write straight into; its measured time is reported (`allreduce_ms`).
    --full: the line also carries the STRONG-scaling form of the legs (`extra.strong_*`: one 4096-ray batch split 4096/N, the global
    ray 0's spacing forwarded to every shard, each with its `allreduce_ms`) -- north_star's ">= 6x strong scaling to 8 GPUs".
  * N = 1, --full: `per_rank_proxy` times what one rank of that 8-GPU job does with its share (512 rays; and the reference's default batch
    of 400 rays, conf/lego.ini:7) + a single-rank RCCL all-reduce, and reports `implied_strong_scaling_8 = t(4096) / (t(512) + allreduce)`.
  * --full: `parity`, the timed configuration rendered once on the golden cfg2 fixture against the REFERENCE's own outputs (max-rel, PSNR);
    at N = 1 also `frame_render` (one 400 x 400 frame) and `cpu_baseline` (the oracle on this host's cores).
  * `n_gpus` in the line is `dist.get_world_size()`, not the flag.
Rank 0 prints ONE JSON line of at most 4 KB (compact_line: the contract's keys, `roofline` and, with --full, `cpu_baseline`, `parity`, a few
scalars of the other legs); the full record -- `extra`, `roofline_phases`, `per_rank_proxy`, `frame_render`, every note -- goes to
bench_extra.json beside this script (--side-file) and, prefixed "bench_extra: ", to stderr.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 1_182_976  # GEMM MACs x 2 of one MLP evaluation
EXEC_FLOP_PER_SAMPLE = FLOP_PER_SAMPLE - 2 * 256 * 256  # executed: point_info (256 x 256) folded into dir_info's feature columns
B, NC, NF = 4096, 64, 128
FLOP_PER_RAY_FWD = FLOP_PER_SAMPLE * (NC + NF)  # 227,131,392
FLOP_PER_RAY_TRAIN = 676_282_368
# backward chain (dX) MACs per sample, SURVEY.md 8(d): coarse pass 557,696, fine pass 588,416 (gamma_p inputs needed for Q9)
CHAIN_FLOP_COARSE, CHAIN_FLOP_FINE = 2 * 557_696, 2 * 588_416
PEAK_F32_MFMA_TFLOPS = 157.3                     # MI355X_MICROARCH.md chip table (fp32 matrix, dense)
PEAK_BF16_MFMA_TFLOPS = 2500.0                   # same table: bf16 matrix, dense (no sparsity)
PEAK_HBM_GBS = 8000.0
N_PARAMS = 593_924
FUSED_TRAIN_STEP = True  # train legs: NeRFModel.train_step (one library call per step); --autograd-step times the three-call autograd path
OVERLAP_ALLREDUCE = False  # set by main(): --overlap / NERF_DP_OVERLAP=1
PROXY_WARMUP_S = 0.2  # untimed run-in of every per_rank_proxy leg (run_leg: warmup_seconds)
RING_ALLREDUCE_MS_ESTIMATE = 0.060  # 30-60 us for the un-overlapped 2.27 MiB SUM all-reduce on an 8-GPU xGMI ring (upper end)


# --------------------------------------------------------------------------------------------------------------------
# launcher (N > 1 without a launcher's environment): no torch.cuda, no HIP before the children exist
# --------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(n, argv):
    """Start n ranks of this script under torch.distributed.run as a CHILD process, relay rank 0's JSON line."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)  # stderr passes through
    out, _ = proc.communicate()
    line = None
    for ln in out.splitlines():
        s = ln.strip()
        if s.startswith("{") and '"metric"' in s:
            try:
                json.loads(s)
                line = s
            except ValueError:
                pass
        elif s:
            print(s, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    if proc.returncode != 0:
        print(f"bench.py: the {n}-rank job exited with code {proc.returncode}", file=sys.stderr)
        return proc.returncode
    if line is None:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        return 1
    return 0


# --------------------------------------------------------------------------------------------------------------------
# synthetic workload
# --------------------------------------------------------------------------------------------------------------------
def synth_inputs(seed, B=None):
    """cfg2: row, col ~ U{0..399}, one lego-like pose, near/far 2/6.  Pure numpy/torch; the
    same generator as oracle.lego_inputs, restated here so the product path never imports the oracle."""
    import numpy as np
    import torch

    B = globals()["B"] if B is None else B
    H = W = 400
    angle = 0.6911112070083618
    focal = 0.5 * W / np.tan(0.5 * angle)
    pose = np.array([[-0.99990219, 0.00419225, -0.01334572, -0.05379832],
                     [-0.01398868, -0.29965907, 0.95394367, 3.84547043],
                     [-4.66e-10, 0.95403719, 0.29968831, 1.20808232]], dtype=np.float64)
    rng = np.random.default_rng(seed)
    row = rng.integers(0, W, size=B)
    col = rng.integers(0, H, size=B)
    m = np.concatenate((pose, np.array([[H], [W], [focal]], dtype=np.float64)), axis=1).flatten()
    pb = np.tile(np.concatenate((m, [2.0, 6.0])), (B, 1))
    K_inv = torch.tensor([[1.0, 0.0, -0.5 * W], [0.0, -1.0, 0.5 * H], [0.0, 0.0, -focal]]).float().t()
    C_true = np.random.default_rng(seed + 1).uniform(0, 1, size=(B, 3)).astype(np.float32)
    return (torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64)), torch.from_numpy(pb), K_inv,
            torch.from_numpy(C_true))


def synth_weights(seed, sharp=False):
    """random-init weights of the reference architecture: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) per tensor (`sharp`: sigma layer x50,
    a peaky density like a trained scene's: the golden fixtures' second weight set)."""
    import math

    import numpy as np
    import torch

    import nerf_tiny_amd as P

    m = P.NeRFModel(NC, NF, B)
    sd = m.state_dict()
    for i, (k, v) in enumerate(sd.items()):
        fan_in = v.shape[1] if v.dim() == 2 else sd[k.replace("bias", "weight")].shape[1]
        bound = 1.0 / math.sqrt(fan_in)
        w = np.random.default_rng([seed, i]).uniform(-bound, bound, size=tuple(v.shape)).astype(np.float32)
        if sharp and "sigma_layer" in k:
            w = w * np.float32(50.0)
        sd[k] = torch.from_numpy(w)
    m.load_state_dict(sd)
    return m


def host_cores():
    """CPU threads this process may really use: min(affinity mask, cgroup cpu.max quota)."""
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except Exception:
        pass
    return cores


def cpu_baseline(seconds_budget=12.0):
    """The oracle (bit-identical restatement of the reference, 'port') timed on this box's host cores on the SAME
    cfg2 workload: one warm-up + as many full 4096-ray forwards as fit the budget (>= 1, <= 3), best time; then the train step
    (forward + loss + backward) on a 1024-ray subset of the same batch, best of 2."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import nerf_oracle as O

    cores = host_cores()
    torch.set_num_threads(cores)
    row, col, pb, K, C_true = O.lego_inputs(B, seed=0)
    params = O.make_weights(0)
    with torch.no_grad():
        O.render(params, row[:256], col[:256], pb[:256], K, NC, NF)  # warm-up (small)
        best, n, t_start = None, 0, time.perf_counter()
        while n < 1 or (time.perf_counter() - t_start) < seconds_budget and n < 3:
            t0 = time.perf_counter()
            O.render(params, row, col, pb, K, NC, NF)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            n += 1
    out = {"value": round(B / best, 1), "unit": "rays/s", "cores": cores, "kind": "port",
           "sample": f"{n} full forward(s) of the same 4096-ray x (64+128) batch, torch CPU fp32, best of {n}; "
                     f"{best:.2f} s/batch"}
    if cores > 8:  # tie back to BASELINE.md section 2 (the reference itself: 967 rays/s on 8 Xeon vCPUs)
        torch.set_num_threads(8)
        with torch.no_grad():
            t0 = time.perf_counter()
            O.render(params, row, col, pb, K, NC, NF)
            out["value_at_8_threads"] = round(B / (time.perf_counter() - t0), 1)
        torch.set_num_threads(cores)
    # train step: forward + loss + backward of the oracle (autograd) on the first 1024 rays of the batch (the full batch needs
    # 12 GB and ~15 s per step; BASELINE.md section 2: 273 rays/s at B = 1024 vs 194 at B = 4096 on 8 Xeon vCPUs)
    bt = 1024
    tb = None
    for _ in range(2):
        t0 = time.perf_counter()
        O.loss_and_grads(params, row[:bt], col[:bt], pb[:bt], K, C_true[:bt], NC, NF)
        dt = time.perf_counter() - t0
        tb = dt if tb is None else min(tb, dt)
    out["train"] = {"value": round(bt / tb, 1), "unit": "rays/s", "cores": cores, "kind": "port",
                    "sample": f"forward + loss + backward (torch autograd, CPU fp32) of the first {bt} rays x (64+128) of the same batch, "
                              f"best of 2; {tb:.2f} s"}
    return out


PMC_FILES = {(False, False): "pmc_latest.json", (True, False): "pmc_train_latest.json", (False, True): "pmc_bf16_fwd_latest.json",
             (True, True): "pmc_bf16_train_latest.json"}  # (train, bf16) -> committed summary under profiles/


PMC_SPLIT_FILE = "pmc_split_fwd_latest.json"
PMC_SPLIT_TRAIN_FILE = "pmc_split_train_latest.json"


def pmc_file(leg):
    if getattr(leg, "split", False):
        return PMC_SPLIT_TRAIN_FILE if leg.train else PMC_SPLIT_FILE
    return PMC_FILES[(leg.train, leg.bf16)]


def read_traffic(leg, kernel_keys, scale=None):
    """HBM bytes per launch from the committed rocprofv3 --pmc summaries (scripts/collect_profiles_r03.sh + scripts/summarize_pmc.py:
    separate FETCH_SIZE / WRITE_SIZE passes, FETCH_SIZE doubled per the gfx950 correction): the mean over `kernel_keys`
    (per-kernel averages over their launches), or with `scale` = {key: launches per step} their sum per step.
    Not measured in this run: the block says so in `traffic_source`."""
    p = os.path.join(ROOT, "profiles", pmc_file(leg))
    try:
        with open(p) as f:
            d = json.load(f)
        vals = [d[k]["hbm_bytes_per_launch"] * (scale[k] if scale else 1) for k in kernel_keys]
        return int(sum(vals) if scale else sum(vals) / len(vals))
    except Exception:
        return None


# --------------------------------------------------------------------------------------------------------------------
# one timed leg
# --------------------------------------------------------------------------------------------------------------------
class Leg:
    def __init__(self, name, train, bf16, split=False):
        self.name, self.train, self.bf16, self.split = name, train, bf16, split  # split: the opt-in split-fp32 inference mode (model.split_mlp)


def run_leg(leg, model, inputs, K, steps, warmup, dist, dev, bucket, time_allreduce=True, warmup_seconds=0.0, profile=True, outputs=None):
    """W untimed + K timed steps of one configuration, bracketed by barrier + synchronize; returns (elapsed s [max over
    ranks], per-kernel HIP-event profile of the library, all-reduce ms per step or None).  time_allreduce=False: no event pair around the
    collective (two markers per step on the stream are not free at a 0.5 ms step).  warmup_seconds: keep warming up (untimed) for that
    long -- the small-batch legs follow 4096-ray fp32 legs in the same process, and a few sub-millisecond steps are not enough for the
    clocks to settle at the lighter load's own level.  profile=False: the library records no HIP events around its kernels (two markers per
    kernel are 3-4 % of a sub-millisecond step; the 4096-ray legs, which the roofline needs live events for, do not notice them).
    outputs: a dict to fill with what the LAST timed step returned to its caller (host float32 copies, taken after the timed region):
    forward C_coarse / C_fine; train step C_coarse / C_fine / loss and one grad_<parameter name> per network tensor."""
    import torch

    from nerf_tiny_amd import _abi

    row, col, pb, C_true = inputs
    model.bf16_mlp = leg.bf16
    model.split_mlp = leg.split and not leg.train
    model.split_train = leg.split and leg.train  # opt-in: the whole train step in split-fp32 arithmetic
    model.grad_bucket = bucket if leg.train else None
    ar_events = []

    def step(timed):
        if leg.train:
            if bucket is None:
                for p in model.network.parameters():
                    p.grad = None
            if FUSED_TRAIN_STEP:  # nerf.py:470-473 (forward, ray_loss, backward) as ONE library call: what NeRFRunner.trainer makes
                res = model.train_step(row, col, pb, K, C_true)
            else:                 # --autograd-step: the reference's three calls through torch.autograd (same kernels)
                Cc, Cf = model(row, col, pb, K)
                loss = model.ray_loss(Cc, Cf, C_true)
                loss.backward()
                res = (Cc, Cf, loss)
            if bucket is not None and dist is not None:  # data-parallel trainer: ONE flat 2.27 MiB SUM all-reduce over RCCL/xGMI
                if timed and time_allreduce:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                bucket.allreduce_sum()
                if timed and time_allreduce:
                    e1.record()
                    ar_events.append((e0, e1))
            elif bucket is not None:
                bucket.consume()  # no collective in this run: the gradients count as used
            return res
        with torch.no_grad():
            return model(row, col, pb, K)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # inference legs run the way NeRFModel.render / display() really render: inside a frozen_weights() section the packed weight image is built
    # by the first call on a workspace and reused afterwards (NERF_HIP_WEIGHTS_UNCHANGED) -- the weights of a rendering loop do not change.
    # Training legs re-pack in every step (the optimizer has changed the weights in between).
    import contextlib

    with (contextlib.nullcontext() if leg.train else model.frozen_weights()):
        for _ in range(max(warmup, 0 if leg.train else 1)):
            step(False)
        if warmup_seconds > 0.0:
            torch.cuda.synchronize()
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < warmup_seconds:
                for _ in range(8):
                    step(False)
                torch.cuda.synchronize()
        fence()
        if profile:
            _abi.profile_begin(steps * 40 + 40)
        t0 = time.perf_counter()
        for _ in range(steps):
            last = step(True)
        fence()
        elapsed = time.perf_counter() - t0
        prof = _abi.profile_end() if profile else {}
        if outputs is not None:  # before any later call can reuse the gradient bucket
            outputs.update((n, t.detach().float().cpu().numpy()) for n, t in zip(("C_coarse", "C_fine", "loss"), last))
            if leg.train:
                outputs.update(("grad_" + n, p.grad.detach().float().cpu().numpy()) for n, p in model.named_parameters())
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ar_ms = (sum(a.elapsed_time(b) for a, b in ar_events) / len(ar_events)) if ar_events else None
    model.grad_bucket = None
    model.split_mlp = model.split_train = False
    return elapsed, prof, ar_ms


def rooflines(leg, prof, b_local, steps):
    """Roofline blocks of one leg from the library's HIP events (recorded on the stream the kernels run on)."""
    peak = PEAK_BF16_MFMA_TFLOPS if leg.bf16 else PEAK_F32_MFMA_TFLOPS
    src = "profiles/" + pmc_file(leg) + " (committed rocprofv3 --pmc passes of this leg; not re-measured in this run)"

    def scaled(t):  # the PMC passes ran at 4096 rays per step; a smaller batch of this run moves proportionally less (the slabs aside)
        return None if t is None else int(t * b_local / B)

    def mfma(kernel, keys, flop_per_launch, traffic_keys, exec_frac):
        """`achieved` / `frac` are the HARDWARE side: the FLOPs the kernel EXECUTES (the folded network) per second against the
        dense MFMA peak -- what the MFMA-busy counter corroborates and what can never exceed 1.  The reference graph's algorithmic FLOPs
        (`flop_per_launch_algorithmic`) over the same time are carried beside it as `achieved_algorithmic` / `frac_algorithmic`
        (= frac / executed_flop_frac; above 1 where the fold removes more work than the kernel loses to its roof)."""
        ms = sum(prof.get(k, (0.0, 0))[0] for k in keys)
        n = sum(prof.get(k, (0.0, 0))[1] for k in keys)
        avg = ms / max(n, 1)
        alg = flop_per_launch / (avg * 1e-3) / 1e12 if avg > 0 else 0.0
        ach = alg * exec_frac
        return {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                "traffic": scaled(read_traffic(leg, traffic_keys)), "traffic_source": src, "kernel": kernel, "avg_launch_ms": round(avg, 4),
                "launches": n, "flop_per_launch": int(round(flop_per_launch * exec_frac)), "flop_per_launch_algorithmic": flop_per_launch,
                "executed_flop_frac": round(exec_frac, 4), "achieved_algorithmic": round(alg, 2), "frac_algorithmic": round(alg / peak, 4)}

    # dominant forward kernel: launched twice per step (coarse pass B*Nc samples, fine pass B*Nf samples); "launch" = the
    # average launch, so that rocprofv3's per-kernel average is directly comparable.  `achieved` / `frac` count the FLOPs the kernels
    # EXECUTE -- 8/9 of the reference network's 1,182,976 per sample: point_info is folded into dir_info (one 128 x 256
    # layer instead of 256 x 256 + 128 x 256) -- so `frac` is a hardware fraction (<= 1); the reference graph's
    # FLOPs over the same time are `achieved_algorithmic` / `frac_algorithmic`.
    def split_block():
        # split-fp32 forward: the fp32 MLP on the bf16 pipe, THREE bf16 MFMAs (hi*hi, hi*mid, mid*hi) per fp32 product.  Roofline = the
        # bf16 MFMA peak against the bf16 FLOPs the kernel executes (3 x the executed fp32 ones); the algorithmic fp32 figure beside it
        ms = sum(prof.get(k, (0.0, 0))[0] for k in ("field_fwd_coarse", "field_fwd_fine"))
        n = sum(prof.get(k, (0.0, 0))[1] for k in ("field_fwd_coarse", "field_fwd_fine"))
        avg = ms / max(n, 1)
        alg = FLOP_PER_SAMPLE * b_local * (NC + NF) // 2
        exe = 3 * EXEC_FLOP_PER_SAMPLE * b_local * (NC + NF) // 2
        ach = exe / (avg * 1e-3) / 1e12 if avg > 0 else 0.0
        return {"bound": "mfma (bf16 pipe)", "achieved": round(ach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_MFMA_TFLOPS, 4),
                "traffic": None if leg.train else scaled(read_traffic(leg, ["k_field_fwd_split"])), "traffic_source": src,
                "kernel": "k_field_fwd_split" + ("<SAVE>" if leg.train else "") + " (average of the coarse- and fine-pass launches)", "avg_launch_ms": round(avg, 4), "launches": n,
                "flop_per_launch": exe, "achieved_algorithmic_fp32": round(alg / (avg * 1e-3) / 1e12, 2) if avg > 0 else 0.0,
                "algorithmic_over_fp32_mfma_peak": round(alg / (avg * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 3) if avg > 0 else 0.0,
                "note": "achieved = executed bf16 MFMA FLOPs (3 per fp32 product of the folded network) against the dense bf16 peak; "
                        "achieved_algorithmic_fp32 = the reference network's fp32 FLOPs (SURVEY.md 8d) per second, above the fp32 MFMA peak because "
                        "the products run on the bf16 pipe with 16-bit-mantissa operands (parity: `parity.split_mlp_vs_reference`)"}

    if getattr(leg, "split", False) and not leg.train:
        return split_block(), None
    fwd_kernel = ("k_field_fwd_bf16<SAVE>" if leg.train else "k_field_fwd_bf16x") if leg.bf16 else ("k_field_fwd_reg<SAVE>" if leg.train else "k_field_fwd_reg")
    fwd_key = (["k_field_fwd_bf16<true, 8>"] if leg.train else ["k_field_fwd_bf16x<2, 8>"]) if leg.bf16 else (["k_field_fwd_reg<true, false>"] if leg.train else ["k_field_fwd"])
    if "render_pair" in prof:  # small bf16-MLP inference batches: ONE launch holds both field passes and both composites of every ray pair
        fwd = mfma("k_render_pair_bf16x (the whole forward of a ray pair per workgroup: both field passes, coarse composite + resampling, merge + sorts + "
                   "composite in one launch)", ("render_pair",), FLOP_PER_SAMPLE * b_local * (NC + NF), fwd_key, EXEC_FLOP_PER_SAMPLE / FLOP_PER_SAMPLE)
        fwd["traffic"] = None  # (no PMC pass of this kernel is committed)
    else:
        fwd = mfma(fwd_kernel + " (average of the coarse- and fine-pass launches)", ("field_fwd_coarse", "field_fwd_fine"),
                   FLOP_PER_SAMPLE * b_local * (NC + NF) // 2, fwd_key, EXEC_FLOP_PER_SAMPLE / FLOP_PER_SAMPLE)
    if getattr(leg, "split", False) and leg.train:
        # the opt-in split-fp32 TRAIN step: forward (field_fwd_split<SAVE>), dX chain (field_bwd_split) on the bf16 pipe with THREE bf16 MFMAs per fp32
        # product -- executed bf16 FLOPs against the dense bf16 peak -- and the weight gradients as the two-part instantiations of the bf16 products
        # (one pass over G_hi, G_mid, X_hi, X_mid): HBM-bound like the bf16 variant's, TWICE its operand bytes
        fwd = split_block()
        fwd["traffic"] = scaled(read_traffic(leg, ["k_field_fwd_split<true>"]))
        cms = sum(prof.get(k, (0.0, 0))[0] for k in ("bwd_field_fine", "bwd_field_coarse"))
        cn = sum(prof.get(k, (0.0, 0))[1] for k in ("bwd_field_fine", "bwd_field_coarse"))
        cavg = cms / max(cn, 1)
        chain_exec_ = 1.0 - 2 * 65536 * (NC + NF) / (CHAIN_FLOP_COARSE * NC + CHAIN_FLOP_FINE * NF)
        calg = (CHAIN_FLOP_COARSE * b_local * NC + CHAIN_FLOP_FINE * b_local * NF) // 2
        cexe = int(3 * calg * chain_exec_)
        cach = cexe / (cavg * 1e-3) / 1e12 if cavg > 0 else 0.0
        chain = {"bound": "mfma (bf16 pipe)", "achieved": round(cach, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(cach / PEAK_BF16_MFMA_TFLOPS, 4),
                 "traffic": scaled(read_traffic(leg, ["k_field_bwd_split<true>", "k_field_bwd_split<false>"])), "traffic_source": src,
                 "kernel": "k_field_bwd_split (dX chain, two-part operands; average of the fine- and coarse-pass launches)", "avg_launch_ms": round(cavg, 4), "launches": cn,
                 "flop_per_launch": cexe, "achieved_algorithmic_fp32": round(calg / (cavg * 1e-3) / 1e12, 2) if cavg > 0 else 0.0}
        dw_ms = prof.get("bwd_dw", (0.0, 0))[0] / max(prof.get("bwd_dw", (0.0, 1))[1], 1)
        wb = ((b_local * NC + 255) // 256 + (b_local * NF + 255) // 256) * 8
        dw_bytes = 2 * DW_BF16_KIB_PER_WAVE_BLOCK * 1024 * wb
        dw = {"bound": "hbm", "achieved": round(dw_bytes / (dw_ms * 1e-3) / 1e9, 1) if dw_ms > 0 else 0.0, "peak": PEAK_HBM_GBS, "unit": "GB/s",
              "frac": round(dw_bytes / (dw_ms * 1e-3) / (PEAK_HBM_GBS * 1e9), 4) if dw_ms > 0 else 0.0,
              "traffic": scaled(read_traffic(leg, list(DW_SPLIT_LAUNCHES), scale=DW_SPLIT_LAUNCHES)), "traffic_source": src,
              "kernel": "k_dw_bf16<.., SPLIT> (the weight-gradient products over two-part operands, one pass + the slab reduce)",
              "avg_launch_ms": round(dw_ms, 4), "launches": prof.get("bwd_dw", (0.0, 0))[1], "bytes_per_launch": dw_bytes}
        for blk in (fwd, chain):
            if blk.get("traffic") and blk["avg_launch_ms"] > 0:
                blk["hbm_gbs"] = round(blk["traffic"] / (blk["avg_launch_ms"] * 1e-3) / 1e9, 1)
                blk["hbm_frac"] = round(blk["hbm_gbs"] / PEAK_HBM_GBS, 4)
        phases = {"forward_with_saves": fwd, "dx_chain": chain, "dw": dw}
        return max(phases.values(), key=lambda b: b["avg_launch_ms"] * (2 if b is not dw else 1)), phases
    fwd["note"] = fwd.get("note") or ("achieved / frac count the FLOPs the kernel EXECUTES (8/9 of the reference network's: point_info folded into dir_info, "
                   "DESIGN.md 3a) -- the MFMA pipe's side, the figure the MFMA-busy counter corroborates; achieved_algorithmic / frac_algorithmic "
                   "price the reference graph's FLOPs (SURVEY.md 8d) over the same time")
    if not leg.train:
        return fwd, None
    sfx = "bf16" if leg.bf16 else "reg"
    chain_exec = 1.0 - 2 * 65536 * (NC + NF) / (CHAIN_FLOP_COARSE * NC + CHAIN_FLOP_FINE * NF)  # the fold removes 65,536 MACs per sample
    chain = mfma(f"k_field_bwd_{sfx} (dX chain; average of the fine- and coarse-pass launches)",
                 ("bwd_field_fine", "bwd_field_coarse"), (CHAIN_FLOP_COARSE * b_local * NC + CHAIN_FLOP_FINE * b_local * NF) // 2,
                 [f"k_field_bwd_{sfx}<true, 8>", f"k_field_bwd_{sfx}<false, 8>"] if leg.bf16 else [f"k_field_bwd_{sfx}<true>", f"k_field_bwd_{sfx}<false>"], chain_exec)
    # weight-gradient phase: all dW = G^T X products of one step (same MACs as one forward over all samples) + slab reduces + thin heads
    dw_ms = prof.get("bwd_dw", (0.0, 0))[0] / max(prof.get("bwd_dw", (0.0, 1))[1], 1)
    launches = DW_BF16_LAUNCHES if leg.bf16 else DW_LAUNCHES
    dw_traffic = scaled(read_traffic(leg, list(launches), scale=launches))
    dw_src = src + "; per step: " + ", ".join(f"{n} x {k}" for k, n in launches.items())
    if leg.bf16:
        # HBM-bound by construction: bytes of bf16 operands per 32-sample wave block, read once each
        wb = ((b_local * NC + 255) // 256 + (b_local * NF + 255) // 256) * 8
        dw_bytes = DW_BF16_KIB_PER_WAVE_BLOCK * 1024 * wb
        dw = {"bound": "hbm", "achieved": round(dw_bytes / (dw_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
              "frac": round(dw_bytes / (dw_ms * 1e-3) / (PEAK_HBM_GBS * 1e9), 4), "traffic": dw_traffic, "traffic_source": dw_src,
              "kernel": "k_dw_bf16 (the weight-gradient passes + slab reduces of one step)", "avg_launch_ms": round(dw_ms, 4),
              "launches": prof.get("bwd_dw", (0.0, 0))[1], "bytes_per_launch": dw_bytes}
    else:
        flop = FLOP_PER_SAMPLE * b_local * (NC + NF)
        ex = EXEC_FLOP_PER_SAMPLE / FLOP_PER_SAMPLE
        alg = flop / (dw_ms * 1e-3) / 1e12 if dw_ms > 0 else 0.0
        dw = {"bound": "mfma", "achieved": round(alg * ex, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(alg * ex / peak, 4),
              "traffic": dw_traffic, "traffic_source": dw_src,
              "kernel": "k_dw4_group / k_dw4 / k_dw_thin / k_dw_reduce / k_fold_grads / k_dir_* (all weight-gradient products of one step incl. the reduce and the thin colour head = one 'launch')",
              "avg_launch_ms": round(dw_ms, 4), "launches": prof.get("bwd_dw", (0.0, 0))[1], "flop_per_launch": int(round(flop * ex)),
              "flop_per_launch_algorithmic": flop, "executed_flop_frac": round(ex, 4), "achieved_algorithmic": round(alg, 2),
              "frac_algorithmic": round(alg / peak, 4)}
    # which roof binds a phase: its measured HBM bytes per launch (PMC, committed) over THIS run's launch time against 8 TB/s, next to
    # the MFMA fraction -- the bf16 training kernels move 2-3 GB per launch and sit closer to the HBM roof than to the matrix one
    for blk in (fwd, chain, dw):
        if blk.get("traffic") and blk["avg_launch_ms"] > 0:
            gbs = blk["traffic"] / (blk["avg_launch_ms"] * 1e-3) / 1e9
            blk["hbm_gbs"] = round(gbs, 1)
            blk["hbm_frac"] = round(gbs / PEAK_HBM_GBS, 4)
            if blk["bound"] == "mfma" and blk["hbm_frac"] > blk["frac"]:
                blk["bound"] = "hbm (by the measured bytes; the MFMA figures are kept in achieved / frac)"
    phases = {"forward_with_saves": fwd, "dx_chain": chain, "dw": dw}
    dominant = max(phases.values(), key=lambda b: b["avg_launch_ms"] * (2 if b is not dw else 1))
    return dominant, phases


# launches of the fp32 weight-gradient phase per train step (dw_f32.hip): the seven 128 x 128-block products (layers 1-7) in ONE launch, the folded
# dpre_dir^T h7 product that carries the sigma head (k_dw4<4, true>), the 128 x 64-block ones (layer 0, layer 4's skip columns), the
# colour head, the reduce, the fold's gradient kernel and the three small kernels of dir_info's direction-encoding columns
DW_LAUNCHES = {"k_dw4_group": 1, "k_dw4<4, true>": 1, "k_dw4<2, false>": 2, "k_dw_thin": 1, "k_dw_reduce": 1, "k_fold_grads": 1,
               "k_dir_prep": 1, "k_dir_gamma_part": 1, "k_dir_gamma_final": 1}
# bf16-MLP variant (dw_bf16.hip), 4096 rays: the six 256 x 256 products in one launch, the products with small blocks (layer 4, layer 0, the
# folded product with the sigma head, the colour head) in another (k_dw_bf16_multi), ONE launch for all slab sums, the fold's gradient kernel
DW_BF16_LAUNCHES = {"k_dw_bf16<8, false, false>": 1, "k_dw_bf16_multi<false>": 1, "k_dw_bf16_reduce_batch": 1, "k_fold_grads": 1}
# the split-fp32 train step: the same products in their two-part instantiations
DW_SPLIT_LAUNCHES = {"k_dw_bf16<8, false, true>": 1, "k_dw_bf16_multi<true>": 1, "k_dw_bf16_reduce_batch": 1, "k_fold_grads": 1}
DW_BF16_KIB_PER_WAVE_BLOCK = 280  # G and X pieces of bf16_common.h over the products (142 + 138 KiB)


def frame_render_block(dev):
    """The reference's display loop (nerf.py:503-520) on one 400 x 400 lego-like frame at the reference's own batch size (BATCH_RAY = 400,
    conf/lego.ini:7): 400 batches of 400 rays in pixel order.  `per_batch` launches one batch per call, as the reference does;
    `fused` is NeRFModel.render -- batches whose ray 0 has the same (near, far) share launches of up to 16,384 rays, every pixel the
    same bits (tests/test_gpu_forward.py::test_render_fuses_batches_bit_identically).  Whole-frame wall time incl. the host side."""
    import torch

    import nerf_tiny_amd as P

    H = W = 400
    _, _, pb1, K, _ = synth_inputs(0, 1)
    rr, cc = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    row, col = rr.reshape(-1).to(dev), cc.reshape(-1).to(dev)
    pb = pb1.float().to(dev).expand(H * W, 17).contiguous()
    m = synth_weights(0, sharp=True).to(dev)
    bm = 400
    m2 = P.NeRFModel(NC, NF, bm).to(dev)
    m2.load_state_dict(m.state_dict())
    out = {"frame": "400 x 400 lego-like view, pixel order, batch_ray 400 (the reference's conf/lego.ini), 64 + 128 samples", "rays": H * W}
    for name, bf16, split in (("f32", False, False), ("f32_split", False, True), ("bf16", True, False)):
        m2.bf16_mlp, m2.split_mlp = bf16, split
        res = {}
        for kind, fuse in (("per_batch", bm), ("fused", 16384)):
            m2.render(row, col, pb, K, 0, 8 * bm, fuse_rays=fuse)  # warm-up (workspace, LDS opt-in)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            _, cf = m2.render(row, col, pb, K, fuse_rays=fuse)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            res[kind] = {"rays_per_s": round(H * W / dt, 1), "ms_per_frame": round(dt * 1e3, 2)}
            res[kind + "_sum"] = float(cf.double().sum())
        res["identical_pixels"] = res.pop("per_batch_sum") == res.pop("fused_sum")
        res["speedup"] = round(res["fused"]["rays_per_s"] / res["per_batch"]["rays_per_s"], 2)
        out[name] = res
    return out


def leg_report(leg, elapsed, prof, ar_ms, steps, warmup, world, b_local, strong):
    rays = b_local * world * steps  # strong: b_local = B / world
    value = rays / elapsed
    flop_ray = FLOP_PER_RAY_TRAIN if leg.train else FLOP_PER_RAY_FWD
    roof, phases = rooflines(leg, prof, b_local, steps)
    rep = {"metric": "rays/sec (64 coarse + 128 fine samples), lego 400x400" + (" [train step: fwd+loss+bwd]" if leg.train else "")
                     + (" [cfg3: bf16 MLP / fp32 composite]" if leg.bf16 else "")
                     + (" [split-fp32 inference: fp32 operands as bf16 hi + mid, 3 bf16 MFMAs per product, fp32 accumulate; same 1e-4 bar]" if getattr(leg, "split", False) and not leg.train else "")
                     + (" [opt-in split-fp32 train step: forward, dX chain and weight gradients with fp32 operands as bf16 hi + mid, 3 bf16 MFMAs per product, fp32 accumulate]" if getattr(leg, "split", False) and leg.train else ""),
           "value": round(value, 1), "unit": "rays/s", "steps": steps, "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 4),
           "dtype": "bf16" if leg.bf16 else ("f32 (bf16 hi+mid split operands, fp32 accumulate)" if getattr(leg, "split", False) else "f32"), "roofline": roof,
           "whole_path_tflops_per_gpu": round(value / world * flop_ray / 1e12, 2),
           "whole_path_frac_of_mfma_peak": round(value / world * flop_ray / 1e12 / (PEAK_BF16_MFMA_TFLOPS if leg.bf16 else PEAK_F32_MFMA_TFLOPS), 4),  # (split leg: of the FP32 peak, i.e. > 1)
           "whole_path_note": "whole_path_* price the ALGORITHMIC FLOPs of the reference graph (SURVEY.md 8d) over the whole step; x 8/9 for the executed side",
           "kernel_ms_per_step": {k: round(v[0] / steps, 4) for k, v in prof.items()}}
    if phases is not None:
        rep["roofline_phases"] = phases
        tr = [(b.get("traffic"), (1 if k == "dw" else 2)) for k, b in phases.items()]
        if all(t for t, _ in tr):  # HBM bytes of the three phases of one step (PMC) over this run's step time
            step_bytes = sum(t * n for t, n in tr)
            rep["step_hbm"] = {"bytes_per_step": int(step_bytes), "achieved_gbs": round(step_bytes / (elapsed / steps) / 1e9, 1), "peak_gbs": PEAK_HBM_GBS,
                               "frac": round(step_bytes / (elapsed / steps) / 1e9 / PEAK_HBM_GBS, 4),
                               "note": "measured HBM traffic of forward-with-saves (x2), dX chain (x2) and the weight-gradient phase, scaled to this run's batch"}
    if leg.train:
        rep["allreduce_ms"] = None if ar_ms is None else round(ar_ms, 4)
        rep["allreduce"] = ((f"SUM all-reduce of {N_PARAMS} fp32 gradients (2.27 MiB) over RCCL, world {world}, " +
                             ("in two parts: point_layer[0..7] on a side stream behind the library's event (beside the last weight-gradient products), the "
                              "rest behind the backward; allreduce_ms = the exposed part" if OVERLAP_ALLREDUCE else
                              "ONE collective behind the step (--overlap / NERF_DP_OVERLAP=1: its early 83 % beside the last weight-gradient products); "
                              "allreduce_ms = HIP events around it in a short second run"))
                            if ar_ms is not None
                            else "none (single rank without a process group)")
    return rep


def parity_block(model, dev):
    """One render of the golden cfg2 case (4096 rays of the 400x400 lego-like view, 64 + 128 samples) with the library, against the
    outputs the REFERENCE itself produced for these inputs and weights (stored in the fixture by tests/golden/make_golden.py, which
    imports /root/reference/nerf.py in the build container).  fp32: the headline path; bf16: the cfg3 variant against the same fp32
    reference outputs.  No oracle code runs here: the fixture is data."""
    import numpy as np
    import torch

    g = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_lego_rand4096.npz"))
    assert int(g["Nc"]) == NC and int(g["Nf"]) == NF and g["row"].shape[0] == B
    m = synth_weights(int(g["seed"]), bool(g["sharp"])).to(dev)  # the fixture stores the generator seed, not the weights
    row, col, pbd = torch.from_numpy(g["row"]).to(dev), torch.from_numpy(g["col"]).to(dev), torch.from_numpy(g["poses_bound"]).float().to(dev)
    K = torch.from_numpy(g["K_inv"])
    ref_c, ref_f = torch.from_numpy(g["C_coarse"]).double(), torch.from_numpy(g["C_fine"]).double()

    def errs(Cc, Cf):
        Cc, Cf = Cc.double().cpu(), Cf.double().cpu()
        mse = float(((Cf - ref_f) ** 2).mean())
        return {"max_rel_C_coarse": float((Cc - ref_c).abs().max() / ref_c.abs().max()), "max_rel_C_fine": float((Cf - ref_f).abs().max() / ref_f.abs().max()),
                "max_elementwise_rel_C_fine": float(((Cf - ref_f).abs() / ref_f.abs().clamp_min(1e-6)).max()),
                "psnr_vs_ref_db": round(10.0 * float(np.log10(1.0 / max(mse, 1e-300))), 2)}

    out = {"fixture": "cfg2_lego_rand4096", "reference": "outputs of /root/reference/nerf.py on the same inputs and weights (tests/golden/make_golden.py)",
           "bar": "max_rel <= 1e-4 (fp32)"}
    with torch.no_grad():
        out.update(errs(*m(row, col, pbd, K)))
        m.split_mlp = True   # the opt-in split-fp32 inference mode: held to the same bar
        out["split_mlp_vs_reference"] = errs(*m(row, col, pbd, K))
        m.split_mlp = False
        m.bf16_mlp = True
        out["bf16_mlp_vs_fp32_reference"] = errs(*m(row, col, pbd, K))
    out["pass"] = bool(out["max_rel_C_coarse"] <= 1e-4 and out["max_rel_C_fine"] <= 1e-4)
    out["split_mlp_vs_reference"]["pass"] = bool(out["split_mlp_vs_reference"]["max_rel_C_coarse"] <= 1e-4 and out["split_mlp_vs_reference"]["max_rel_C_fine"] <= 1e-4)
    for k in ("max_rel_C_coarse", "max_rel_C_fine", "max_elementwise_rel_C_fine"):
        out[k] = float(f"{out[k]:.3e}")
        for sub in ("bf16_mlp_vs_fp32_reference", "split_mlp_vs_reference"):
            out[sub][k] = float(f"{out[sub][k]:.3e}")
    return out



# --------------------------------------------------------------------------------------------------------------------
# the result line: compact (<= LINE_LIMIT bytes) for the driver; the full record goes to bench_extra.json beside this script
# --------------------------------------------------------------------------------------------------------------------
LINE_LIMIT = 4096
DUMP_LIMIT = 64 << 20  # --dump-outputs: bytes in all
SIDE_FILE = "bench_extra.json"


def write_side_file(full, explicit=None):
    """The full record of the run (every leg, roofline phases, per-rank proxy, frame render, notes) as JSON: at `explicit` (--side-file), else
    beside bench.py and -- when that directory exists, so that it travels back from a gpurun box -- under gpurun_out/.  Returns the first
    path written, or None (the record is on stderr as well)."""
    path = None
    targets = [explicit] if explicit else [os.path.join(ROOT, SIDE_FILE)] + (
        [os.path.join(ROOT, "gpurun_out", SIDE_FILE)] if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else [])
    for t in targets:
        try:
            with open(t, "w") as f:
                json.dump(full, f, indent=1)
            path = path or t
        except OSError as ex:
            print(f"bench.py: could not write {t}: {ex}", file=sys.stderr)
    return path


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(full, side_path=None):
    """The ONE line the driver parses: the contract's keys, `roofline` and `cpu_baseline` as prompt section 4 defines them, the parity of
    the timed configuration and a handful of scalars of the other legs.  No notes, no per-kernel tables, no nested legs: those are in the
    side file.  Free-text values are cut to 160 characters; the result is asserted to fit LINE_LIMIT bytes."""

    def cut(v, n=160):
        return v if not isinstance(v, str) or len(v) <= n else v[: n - 3] + "..."

    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"))
    line["metric"] = cut(line.get("metric"), 120)
    cfg = full.get("config", {})
    line["config"] = {k: cut(cfg[k]) for k in ("workload", "rays_per_step_per_gpu", "mode", "weights", "parallelism") if k in cfg}
    line["roofline"] = {k: cut(v, 100) for k, v in _pick(full.get("roofline", {}), (
        "bound", "achieved", "peak", "unit", "frac", "frac_algorithmic", "traffic", "traffic_source", "kernel", "avg_launch_ms", "launches")).items()}
    if "cpu_baseline" in full:
        cb = full["cpu_baseline"]
        line["cpu_baseline"] = {k: cut(v, 120) for k, v in _pick(cb, ("value", "unit", "cores", "kind", "sample", "value_at_8_threads")).items()}
        if isinstance(cb.get("train"), dict):
            line["cpu_baseline"]["train_value"] = cb["train"].get("value")
        line["gpu_over_cpu"] = full.get("gpu_over_cpu")
    par = full.get("parity")
    if isinstance(par, dict):
        line["parity"] = _pick(par, ("max_rel_C_coarse", "max_rel_C_fine", "psnr_vs_ref_db", "pass", "error"))
        if "error" in line["parity"]:
            line["parity"]["error"] = cut(line["parity"]["error"])
    if "allreduce_ms" in full:
        line["allreduce_ms"] = full["allreduce_ms"]
    ex = full.get("extra", {})
    for name in ("train_f32", "forward_bf16", "train_bf16", "forward_f32_split", "train_f32_split"):
        if name in ex:
            line[name + "_rays_per_s"] = ex[name].get("value")
    for name in ("train_f32", "train_bf16"):  # the N > 1 strong-scaling legs: one 4096-ray batch split over the ranks
        if "strong_" + name in ex:
            line["strong_" + name + "_rays_per_s"] = ex["strong_" + name].get("value")
            line["strong_" + name + "_allreduce_ms"] = ex["strong_" + name].get("allreduce_ms")
    if "strong_forward_f32" in ex:
        line["strong_forward_f32_rays_per_s"] = ex["strong_forward_f32"].get("value")
    if "strong_forward_bf16" in ex:
        line["strong_forward_bf16_rays_per_s"] = ex["strong_forward_bf16"].get("value")
    ph = full.get("extra", {}).get("train_f32", {}).get("roofline_phases") or full.get("roofline_phases")
    if isinstance(ph, dict):
        line["train_f32_phase_frac"] = {k: v.get("frac") for k, v in ph.items() if isinstance(v, dict)}
    imp = full.get("implied_strong_scaling_8")
    if isinstance(imp, dict) and imp:
        line["implied_strong_scaling_8_min"] = min(imp.values())
        ring = full.get("implied_strong_scaling_8_with_ring_estimate")
        if isinstance(ring, dict) and ring:
            line["implied_strong_scaling_8_with_ring_estimate_min"] = min(ring.values())
    if "rehearsal" in full:
        line["rehearsal"] = cut(full["rehearsal"], 120)
    if side_path is not None:
        line["side_file"] = os.path.basename(side_path)
    n = len(json.dumps(line, separators=(",", ":")))
    if n > LINE_LIMIT:  # never print a line the driver cannot take: drop the optional scalars, keep the contract + roofline + cpu_baseline
        for k in [k for k in line if k.endswith("_rays_per_s") or k.startswith("implied_") or k in ("train_f32_phase_frac", "parity", "gpu_over_cpu")]:
            line.pop(k)
        n = len(json.dumps(line, separators=(",", ":")))
    assert n <= LINE_LIMIT, f"bench.py: result line is {n} bytes (> {LINE_LIMIT})"
    return line


# --------------------------------------------------------------------------------------------------------------------
def dry_main(args):
    """CPU rehearsal of the N-rank plumbing (tests/test_bench_launch.py): gloo ranks, the same fence / MAX reduction /
    flat-bucket all-reduce, NO kernels -- the line is marked "dry" and carries no throughput."""
    import torch
    import torch.distributed as dist

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    dist.init_process_group("gloo")
    if os.environ.get("BENCH_TEST_FAIL_RANK") == str(rank):  # tests/test_bench_launch.py: a dying rank must fail the whole job
        os._exit(3)
    flat = torch.full((N_PARAMS,), float(rank + 1))
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.fill_(float(rank + 1))
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": "dry run (gloo, no kernels)", "value": 0.0, "unit": "rays/s", "n_gpus": dist.get_world_size(),
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(float(t) / max(args.steps, 1) * 1e3, 4),
                          "dry": True, "flag_gpus": args.gpus}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=["forward", "train"], default="forward")
    ap.add_argument("--mlp", choices=["f32", "bf16"], default="f32",
                    help="f32 = the headline metric (reference precision); bf16 = BASELINE.json cfg3 'bf16 MLP / fp32 composite' "
                         "(NOT the headline: reduced precision, reported as its own metric)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default, the driver's contract): every rank renders its own 4096-ray batches; strong: ONE 4096-ray "
                         "batch is split into contiguous slices of 4096/N rays (SURVEY.md 8d cfg3), with the global ray 0's (near, far) "
                         "handed to every rank (quirk Q6)")
    ap.add_argument("--split", action="store_true",
                    help="forward only: the opt-in split-fp32 inference mode (model.split_mlp) as the leg of the line (profiling runs; NOT the "
                         "driver's headline, which stays the exact-fp32 path)")
    ap.add_argument("--autograd-step", action="store_true",
                    help="train legs: forward, ray_loss, backward as three calls through torch.autograd (the reference's call surface) instead of "
                         "NeRFModel.train_step, the one library call NeRFRunner.trainer makes (same kernels, same results)")
    ap.add_argument("--overlap", action="store_true", help="N > 1 train legs: overlap the early part of the all-reduce with the last weight-gradient products")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline leg: the other legs (and at N > 1 their strong-scaling form), at N = 1 the per-rank proxy, "
                         "a 400 x 400 frame and the CPU baseline, and the parity check against the reference's outputs.  Without it the "
                         "run times the headline leg alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full without the other legs, proxy, frame and parity (profiling runs)")
    ap.add_argument("--side-file", default=None, help="where the full record goes (default: bench_extra.json beside this script); the stdout line "
                                                      "is the compact <= 4 KB form of it")
    ap.add_argument("--dry", action="store_true", help="CPU rehearsal of the launcher + process group over gloo (no kernels; tests only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline leg's last timed step returned (rank 0) as DIR/<name>.npy, float32: "
                         "C_coarse, C_fine [4096, 3]; train: also loss and grad_<parameter> (2.4 MB).  Inputs and weights are seeded: "
                         "two runs with the same arguments see the same inputs")
    args = ap.parse_args()

    global FUSED_TRAIN_STEP
    FUSED_TRAIN_STEP = not args.autograd_step
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.gpus > 1 and "RANK" not in os.environ:
        # parent of an N-rank job: nothing below this line runs here, in particular no torch.cuda / HIP call
        return launch_ranks(args.gpus, sys.argv[1:])
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if "RANK" in os.environ and world_env != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started WORLD_SIZE={world_env} ranks")
    if args.dry:
        return dry_main(args)

    import torch

    import nerf_tiny_amd as P
    from nerf_tiny_amd import _abi

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    _abi.lib()  # fail loudly if the HIP library is missing
    # BENCH_DIST_BACKEND=gloo (tests only): rehearse the N-rank code path -- sharding, global ray 0, strong legs, MAX reduction, the compact line
    # with its strong_* scalars -- with N ranks SHARING the GPUs there are (RCCL refuses two ranks on one device; gloo moves the bucket through
    # the host).  The line it prints measures nothing and is marked "rehearsal".
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    if backend == "gloo":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    saved_stdout = None
    if world_env > 1 or os.environ.get("BENCH_FORCE_DIST") == "1":  # the latter: rehearse the RCCL path with a single rank
        # RCCL prints a version banner on fd 1; the contract is ONE JSON line on stdout, so native stdout goes to stderr
        # until the result is printed
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))  # only the single-rank rehearsal comes without a launcher's environment
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    world = dist.get_world_size() if dist is not None else 1

    strong = args.scaling == "strong"
    row, col, pb, K, C_true = synth_inputs(seed=1000 + (0 if strong else rank))
    model = synth_weights(seed=0).to(dev)
    # the flat gradient buffer of the data-parallel trainer: the backward kernels write into views of it (no pack / unpack)
    bucket = P.parallel.GradBucket(model.network.parameters())
    # --overlap / NERF_DP_OVERLAP=1: the all-reduce of point_layer[0..7] (83 % of the bytes) on a side stream beside the last weight-gradient
    # products (GradBucket.enable_overlap).  Off by default: on one rank the split launches and the two cross-stream hand-offs cost 46-62 us
    # per step (scripts/dp_step_proxy.py), as much as an 8-rank ring all-reduce of 2.27 MiB is priced at
    if dist is not None and (args.overlap or os.environ.get("NERF_DP_OVERLAP") == "1"):
        bucket.enable_overlap()
        global OVERLAP_ALLREDUCE
        OVERLAP_ALLREDUCE = True

    def shard(full, lo, hi):
        """Device inputs of rays [lo, hi) of a batch; the model is told its batch size and the GLOBAL ray 0's (near, far): its
        coarse spacing goes to every shard (nerf.py:233, quirk Q6)."""
        r, c, p_, ct = full
        model.batch_ray = hi - lo
        model.ray0_near_far = (float(p_[0, 15]), float(p_[0, 16])) if lo > 0 else None
        return (r[lo:hi].to(dev), c[lo:hi].to(dev), p_[lo:hi].float().to(dev), ct[lo:hi].to(dev))

    full = (row, col, pb, C_true)
    b_local = B
    if strong:
        if B % world:
            raise SystemExit(f"--scaling strong needs {B} % N == 0")
        b_local = B // world
    inputs = shard(full, rank * b_local, (rank + 1) * b_local) if strong else shard(full, 0, B)

    if args.split and args.mlp == "bf16":
        raise SystemExit("--split is the split-fp32 mode (inference: model.split_mlp, train step: model.split_train): not with --mlp bf16")
    head = Leg("headline", args.mode == "train", args.mlp == "bf16", args.split)
    dumped = {} if args.dump_outputs else None
    elapsed, prof, ar_ms = run_leg(head, model, inputs, K, args.steps, args.warmup, dist, dev, bucket, outputs=dumped)
    if dumped is not None and rank == 0:
        import numpy as np

        assert sum(a.nbytes for a in dumped.values()) <= DUMP_LIMIT, "bench.py: --dump-outputs would write more than 64 MB"
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dumped.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    rep = leg_report(head, elapsed, prof, ar_ms, args.steps, args.warmup, world, b_local, strong)
    # everything below that runs more kernels, or the CPU oracle, is --full's: a plain run ends with the headline leg
    more = args.full and not args.no_extra
    extra = {}
    # (name, train, bf16, timed steps, warm-up steps): every leg is timed over >= 0.1 s
    legs = (("forward_f32", False, False, 20, 3), ("train_f32", True, False, 8, 2), ("forward_bf16", False, True, 160, 8), ("train_bf16", True, True, 40, 4),
            ("forward_f32_split", False, False, 60, 4), ("train_f32_split", True, False, 8, 2))
    def brief(r, rays_per_step):
        return {k: r[k] for k in ("value", "unit", "ms_per_step", "ms_per_step_with_kernel_events", "steps", "dtype", "kernel_ms_per_step", "allreduce_ms") if k in r} | {
            "rays_per_step": rays_per_step, "roofline_frac": r["roofline"]["frac"], "roofline_frac_algorithmic": r["roofline"].get("frac_algorithmic"),
            "whole_path_frac_of_mfma_peak": r["whole_path_frac_of_mfma_peak"]}

    def measured(leg, inp, k, w, d, world_, b_loc, strong_, run_in=0.0):
        """A leg that is not the headline: K steps timed WITHOUT the library's per-kernel HIP events (two markers around each of a step's
        7-20 kernels: 0.2 % of the fp32 legs, 2.5 % of a 4096-ray bf16 train step, 5 % of a 512-ray one), then a short run WITH them for
        kernel_ms_per_step, the roofline blocks and allreduce_ms.  (The headline leg keeps the contract's form: K steps, events live.)"""
        e, _, _ = run_leg(leg, model, inp, K, k, w, d, dev, bucket, time_allreduce=False, warmup_seconds=run_in, profile=False)
        kp = max(k // 4, 4)
        ep, pp, ap = run_leg(leg, model, inp, K, kp, 1, d, dev, bucket)
        r = leg_report(leg, ep, pp, ap, kp, w, world_, b_loc, strong_)
        ms = e / k * 1e3
        scale = (ep / kp * 1e3) / ms
        r["ms_per_step_with_kernel_events"], r["ms_per_step"], r["steps"] = r["ms_per_step"], round(ms, 4), k
        r["value"] = round(r["value"] * scale, 1)
        r["whole_path_tflops_per_gpu"] = round(r["whole_path_tflops_per_gpu"] * scale, 2)
        r["whole_path_frac_of_mfma_peak"] = round(r["whole_path_frac_of_mfma_peak"] * scale, 4)
        if "step_hbm" in r:
            r["step_hbm"]["achieved_gbs"] = round(r["step_hbm"]["achieved_gbs"] * scale, 1)
            r["step_hbm"]["frac"] = round(r["step_hbm"]["frac"] * scale, 4)
        return r

    if more:
        for name, train, bf16, k, w in legs:
            split = name.endswith("_split")
            if (train, bf16, split) == (head.train, head.bf16, head.split):
                continue
            extra[name] = measured(Leg(name, train, bf16, split), inputs, k, w, dist, world, b_local, strong)

    # ---- N > 1: the STRONG-scaling form of the same legs in the same line (north_star: ">= 6x strong scaling to 8 GPUs"): ONE 4096-ray
    # batch (the same on every rank) split into contiguous slices of 4096 / N rays, the global ray 0's spacing forwarded, one flat SUM
    # all-reduce per train step where the reference has loss.backward(); optimizer.step() (nerf.py:473-474)
    if dist is not None and not strong and more and B % world == 0:  # (also in the single-rank RCCL rehearsal: same code path)
        g_full = synth_inputs(seed=1000)
        g_full = (g_full[0], g_full[1], g_full[2], g_full[4])
        bs = B // world
        s_in = shard(g_full, rank * bs, (rank + 1) * bs)
        for name, train, bf16, k, w in legs:
            leg = Leg(name, train, bf16, name.endswith("_split"))
            extra["strong_" + name] = brief(measured(leg, s_in, 3 * k, w + 2, dist, world, bs, True), B)
        inputs = shard(full, 0, B)

    # ---- N = 1: what ONE rank of an 8-GPU strong-scaling job does with its share, measured here: 512 rays (4096 / 8) and the reference's
    # own default batch of 400 rays (conf/lego.ini:7), the first rays of the same batch (global ray 0 = local ray 0)
    proxy = None
    if world == 1 and dist is None and not strong and more:
        proxy = {}
        t_full = {name: (rep["ms_per_step"] if (train, bf16, name.endswith("_split")) == (head.train, head.bf16, head.split) else extra[name]["ms_per_step"])
                  for name, train, bf16, _, _ in legs}
        # a REAL (single-rank) RCCL group for the collective a rank adds per train step
        try:
            sys.stdout.flush()
            saved_stdout = os.dup(1)
            os.dup2(2, 1)
            import torch.distributed as dist

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            dist.init_process_group("nccl", device_id=dev)
        except Exception as ex:  # no RCCL on this box: the proxy then carries no collective
            print(f"bench.py: single-rank RCCL group not available: {ex}", file=sys.stderr)
            dist = None
        # the numerator under the same conditions as the denominators: the full 4096-ray step of every leg once more, without kernel events
        proxy["4096"] = {}
        for name, train, bf16, k, w in legs:
            leg = Leg(name, train, bf16, name.endswith("_split"))
            e, _, _ = run_leg(leg, model, inputs, K, k, w, None, dev, bucket, warmup_seconds=PROXY_WARMUP_S, profile=False)
            with_ev = rep["ms_per_step"] if name not in extra else extra[name]["ms_per_step_with_kernel_events"]  # (the headline leg IS timed with them)
            proxy["4096"][name] = {"ms_per_step": round(e / k * 1e3, 4), "ms_per_step_with_kernel_events": with_ev, "steps": k, "rays_per_step": B}
            t_full[name] = proxy["4096"][name]["ms_per_step"]
        for bs in (512, 400):
            s_in = shard(full, 0, bs)
            proxy[str(bs)] = {}
            for name, train, bf16, k, w in legs:
                leg = Leg(name, train, bf16, name.endswith("_split"))
                kk = 4 * k
                proxy[str(bs)][name] = brief(measured(leg, s_in, kk, w + 3, None, 1, bs, True, PROXY_WARMUP_S), bs)
                if train and dist is not None:
                    # the step a data-parallel rank really makes: the same call + the flat 2.27 MiB SUM all-reduce on the RCCL group behind
                    # it, timed as ONE loop (the collective's enqueue overlaps the kernels of the step, as it does in NeRFRunner.trainer)
                    e2, _, _ = run_leg(leg, model, s_in, K, kk, w + 3, dist, dev, bucket, time_allreduce=False, warmup_seconds=PROXY_WARMUP_S, profile=False)
                    proxy[str(bs)][name]["dp_step_ms_single_rank"] = round(1e3 * e2 / kk, 4)
        inputs = shard(full, 0, B)
        # ... and the collective ALONE, back to back (host-bound: the enqueue rate of an empty queue, not what a step pays)
        ar1 = None
        if dist is not None:
            try:
                bucket.pending = False
                for _ in range(5):
                    bucket.allreduce_sum()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    bucket.allreduce_sum()
                e1.record()
                torch.cuda.synchronize()
                ar1 = e0.elapsed_time(e1) / 50
            except Exception as ex:
                print(f"bench.py: single-rank RCCL all-reduce not measured: {ex}", file=sys.stderr)
        proxy["allreduce_ms_single_rank"] = None if ar1 is None else round(ar1, 4)

        def implied(ar_ms):
            """t(4096 rays) / t(a rank's 512-ray step incl. its collective).  ar_ms None: the MEASURED data-parallel step on the single-rank
            RCCL group (dp_step_ms_single_rank; falls back to t(512) + the stand-alone all-reduce); a number: t(512) + that estimate."""
            out_ = {}
            for name, train, _, _, _ in legs:
                t512 = proxy["512"][name]["ms_per_step"]
                if train:
                    t512 = (proxy["512"][name].get("dp_step_ms_single_rank") or t512 + (ar1 or 0.0)) if ar_ms is None else t512 + ar_ms
                out_[name] = round(t_full[name] / t512, 2)
            return out_

        # UPPER BOUND: the collective inside this figure ran on a single-rank RCCL group (launch + kernel, no xGMI hop, no straggler)
        proxy["implied_strong_scaling_8"] = implied(None)
        # ... and with an 8-rank ring's latency in its place.  Not measured (no 8-GPU node was available to any round so far): SURVEY.md 8e
        # prices the un-overlapped 2.27 MiB SUM all-reduce at 30-60 us (latency-bound: 7 xGMI hops x 2 phases; the bytes are 15 us of one
        # link); the upper end is used, all of it exposed
        proxy["ring_allreduce_ms_estimate"] = RING_ALLREDUCE_MS_ESTIMATE
        proxy["implied_strong_scaling_8_with_ring_estimate"] = implied(RING_ALLREDUCE_MS_ESTIMATE)
        proxy["note"] = ("implied_strong_scaling_8 = t(4096 rays) / t(512 rays), both timed without the library's per-kernel events after a 0.2 s run-in "
                         "(per_rank_proxy.4096 / .512); for the train legs t(512) is dp_step_ms_single_rank = the measured "
                         "step of a data-parallel rank (NeRFModel.train_step + the flat SUM all-reduce behind it on a single-rank RCCL group, timed as "
                         "one loop), all in this run on one GPU: an UPPER BOUND (no xGMI hops, no straggler).  allreduce_ms_single_rank is the same "
                         "collective alone, back to back (host-bound enqueue; inside a step it hides behind the kernels).  "
                         "implied_strong_scaling_8_with_ring_estimate = t(4096) / (t(512) + a documented "
                         f"{RING_ALLREDUCE_MS_ESTIMATE * 1e3:.0f} us estimate of the exposed 8-rank ring all-reduce, SURVEY.md 8e); the 8-GPU "
                         "number itself is extra.strong_* of the driver's N = 8 line")

    # ---- parity of the timed configuration, in the line: the reference's OWN outputs for cfg2 (tests/golden/cfg2_lego_rand4096.npz: inputs,
    # weight seed and the C_coarse / C_fine the reference returned in the build container) against this library's render of the same
    parity = None
    if rank == 0 and more:
        try:
            parity = parity_block(model, dev)
        except Exception as ex:
            parity = {"error": str(ex)}

    if rank == 0:
        out = {
            "metric": rep["metric"], "value": rep["value"], "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": rep["ms_per_step"], "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": rep["dtype"], "data": "synthetic",
            "config": {"workload": ("cfg3: lego-like 400x400 view, 4096-ray batches, 64 coarse + 128 fine samples, bf16 MLP (fp32 accumulate) / fp32 "
                                    "everything else, " if head.bf16 else
                                    "cfg2: lego-like 400x400 view, 4096-ray batches, 64 coarse + 128 fine samples, fp32, ")
                                   + "random-init 8x256 NeRF MLP (593,924 params)", "rays_per_step_per_gpu": b_local,
                       "mode": args.mode,
                       "train_step": ("NeRFModel.train_step: forward + ray_loss + backward in one library call, as NeRFRunner.trainer does"
                                      if FUSED_TRAIN_STEP else "three calls through torch.autograd (the reference's call surface)"),
                       "weights": ("re-packed every step (the optimizer changes them)" if head.train else
                                   "packed once per rendering loop (NeRFModel.frozen_weights, the form render() / display() use)"),
                       "parallelism": f"ray-batch x{world} (independent batches, no collective)" if not head.train else
                       f"ray-batch DP x{world} (one flat SUM all-reduce of 593,924 fp32 gradients per step)"},
            "roofline": rep["roofline"],
            "whole_path_tflops": rep["whole_path_tflops_per_gpu"],  # per GPU
            **({"rehearsal": "BENCH_DIST_BACKEND=gloo: ranks share the GPU(s), the collective goes through the host -- the code path, not a measurement"}
               if backend == "gloo" and dist is not None else {}),
            "kernel_ms_per_step": rep["kernel_ms_per_step"],
        }
        for k in ("roofline_phases", "allreduce_ms", "allreduce"):
            if k in rep:
                out[k] = rep[k]
        if parity is not None:
            out["parity"] = parity
        if extra:
            out["extra"] = extra
        if world == 1 and more:
            try:
                out["frame_render"] = frame_render_block(dev)
            except Exception as ex:
                out["frame_render"] = {"error": str(ex)}
        if proxy is not None:
            out["per_rank_proxy"] = proxy
            out["implied_strong_scaling_8"] = proxy["implied_strong_scaling_8"]  # upper bound: see per_rank_proxy.note
            out["implied_strong_scaling_8_with_ring_estimate"] = proxy["implied_strong_scaling_8_with_ring_estimate"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            cb = cpu_baseline()
            out["cpu_baseline"] = cb
            out["gpu_over_cpu"] = round(rep["value"] / cb["value"], 1)
            if "train_f32" in extra and "train" in cb:
                out["gpu_over_cpu_train"] = round(extra["train_f32"]["value"] / cb["train"]["value"], 1)
        if saved_stdout is not None:
            sys.stdout.flush()
            os.dup2(saved_stdout, 1)
        # the driver reads ONE short line (BENCH_r04: a 21 KB line was not taken); everything else goes to the side file and to stderr
        side = write_side_file(out, args.side_file)
        line = compact_line(out, side)
        print("bench_extra: " + json.dumps(out), file=sys.stderr, flush=True)  # (prefixed: never mistaken for the result line)
        print(json.dumps(line, separators=(",", ":")), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
