"""GPU: the RCCL leg of the multi-GPU path, run for real on the one GPU of the box in FRESH child processes (a process group per
child; never re-exec'd from a process that has initialised the GPU).  The N-rank launcher itself is covered on CPU by
tests/test_bench_launch.py; sharding arithmetic by tests/test_parallel_gloo.py."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


@pytest.mark.timeout(600)
def test_train_step_sharded_over_rccl_single_rank():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "rccl_single_rank.py")], capture_output=True, text=True,
                       env=_env(), timeout=560)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "RCCL-OK" in r.stdout


@pytest.mark.timeout(900)
def _bench(args, env, tmp_path):
    """bench.py as the driver runs it: ONE stdout line of at most 4 KB (the compact record) + the full record in the side file."""
    side = os.path.join(str(tmp_path), "bench_extra.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--side-file", side], capture_output=True, text=True, env=env, timeout=860)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    assert len(lines[0]) < 4096, len(lines[0])  # BENCH_r04: a 21 KB line was not taken by the driver
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline"):
        assert k in line, k
    assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms", "launches"}
    assert "bench_extra: {" in r.stderr  # the full record is on stderr as well
    with open(side) as f:
        full = json.load(f)
    for k in ("metric", "value", "ms_per_step", "n_gpus", "dtype"):
        assert line[k] == full[k], k
    assert line["roofline"]["frac"] == full["roofline"]["frac"]
    return line, full


@pytest.mark.timeout(900)
def test_bench_train_leg_with_rccl_allreduce(tmp_path):
    """bench.py's data-parallel train leg with a real (1-rank) RCCL group: one compact JSON line, n_gpus from the process group, the
    all-reduce measured, and (side file) every extra leg present with its own roofline block."""
    env = _env()
    env["BENCH_FORCE_DIST"] = "1"
    line, out = _bench(["--mode", "train", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"], env, tmp_path)
    assert out["n_gpus"] == 1 and out["config"]["mode"] == "train"
    assert line["allreduce_ms"] == out["allreduce_ms"] and line["parity"]["pass"] is True
    assert line["strong_train_bf16_rays_per_s"] == out["extra"]["strong_train_bf16"]["value"]
    assert out["allreduce_ms"] is not None and 0.0 < out["allreduce_ms"] < 50.0
    assert set(out["roofline_phases"]) == {"forward_with_saves", "dx_chain", "dw"}
    # the weak legs and -- the code path of the driver's N = 8 line -- the strong-scaling form of all four legs (here: one rank = the whole batch)
    assert set(out["extra"]) == {"forward_f32", "forward_bf16", "train_bf16", "forward_f32_split", "train_f32_split", "strong_forward_f32", "strong_train_f32",
                                 "strong_forward_bf16", "strong_train_bf16", "strong_forward_f32_split", "strong_train_f32_split"}
    for name, leg in out["extra"].items():
        if name.startswith("strong_"):
            # `roofline.frac` is a HARDWARE fraction (executed FLOPs or measured bytes over the peak): never above 1
            assert leg["value"] > 0 and leg["rays_per_step"] == 4096 and 0.0 < leg["roofline_frac"] <= 1.0
        else:
            assert leg["value"] > 0 and 0.0 < leg["roofline"]["frac"] <= 1.0
            if "frac_algorithmic" in leg["roofline"]:  # the reference graph's FLOPs over the same time: 9/8 of the executed ones (the fold)
                assert leg["roofline"]["frac"] < leg["roofline"]["frac_algorithmic"] < 1.125
    assert 0.0 < out["roofline"]["frac"] <= 1.0
    for ph in out["roofline_phases"].values():
        assert 0.0 < ph["frac"] <= 1.0
    assert out["extra"]["train_bf16"]["allreduce_ms"] is not None
    assert out["extra"]["strong_train_f32"]["allreduce_ms"] is not None and out["extra"]["strong_train_bf16"]["allreduce_ms"] is not None
    assert out["parity"]["pass"] is True and out["parity"]["split_mlp_vs_reference"]["pass"] is True


@pytest.mark.timeout(900)
def test_bench_default_line_carries_the_per_rank_proxy(tmp_path):
    """The full run (`python bench.py --full`, N = 1; fewer steps here): one compact JSON line with roofline + parity; the side file holds
    the per-rank proxy of the 8-GPU strong-scaling step -- a rank's 512-ray share and the reference's 400-ray batch, the train legs also as the
    MEASURED data-parallel step (train_step + the flat SUM all-reduce behind it on a single-rank RCCL group) that `implied_strong_scaling_8` is
    computed from."""
    line, out = _bench(["--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"], _env(), tmp_path)
    assert out["n_gpus"] == 1 and out["dtype"] == "f32" and 0.0 < out["roofline"]["frac"] <= 1.0 and out["parity"]["pass"] is True
    assert line["parity"]["pass"] is True and line["implied_strong_scaling_8_min"] == min(out["implied_strong_scaling_8"].values())
    assert line["train_f32_rays_per_s"] == out["extra"]["train_f32"]["value"] and line["train_bf16_rays_per_s"] == out["extra"]["train_bf16"]["value"]
    px = out["per_rank_proxy"]
    for bs in ("512", "400"):
        assert set(px[bs]) == {"forward_f32", "train_f32", "forward_bf16", "train_bf16", "forward_f32_split", "train_f32_split"}
        for name, leg in px[bs].items():
            assert leg["rays_per_step"] == int(bs) and leg["ms_per_step"] > 0 and 0.0 < leg["roofline_frac"] <= 1.0
            if name.startswith("train"):
                # the collective rides behind the step's kernels: the data-parallel step is the plain step plus a few microseconds
                assert leg["ms_per_step"] * 0.9 < leg["dp_step_ms_single_rank"] < leg["ms_per_step"] + 0.08, (name, leg)
    assert px["allreduce_ms_single_rank"] is not None and 0.0 < px["allreduce_ms_single_rank"] < 1.0
    imp, ring = out["implied_strong_scaling_8"], out["implied_strong_scaling_8_with_ring_estimate"]
    assert set(imp) == set(px["512"]) and all(1.0 < v <= 8.5 for v in imp.values()), imp
    for name in imp:  # the ring estimate only ever lowers a train figure and leaves the inference figures alone
        assert ring[name] <= imp[name] + 1e-9 and (name.startswith("train") or ring[name] == imp[name])
    assert imp["train_f32"] == round(px["4096"]["train_f32"]["ms_per_step"] / px["512"]["train_f32"]["dp_step_ms_single_rank"], 2)
    assert imp["forward_bf16"] == round(px["4096"]["forward_bf16"]["ms_per_step"] / px["512"]["forward_bf16"]["ms_per_step"], 2)
    for name, leg in px["4096"].items():  # the same step with and without the library's kernel events: within a few per cent
        assert 0.9 * leg["ms_per_step_with_kernel_events"] < leg["ms_per_step"] < 1.05 * leg["ms_per_step_with_kernel_events"], (name, leg)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["forward", "train"])
def test_bench_plain_run_times_the_headline_leg_alone(tmp_path, mode):
    """The driver's command without --full: the headline leg with its own roofline (and, for the train step, its phases) from the HIP events
    of its timed steps, and nothing else -- no other legs, no per-rank proxy, no frame, no parity, no CPU baseline."""
    line, full = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--mode", mode], _env(), tmp_path)
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["mode"] == mode and line["dtype"] == "f32" and 0.0 < line["roofline"]["frac"] <= 1.0
    assert (set(full.get("roofline_phases", {})) == {"forward_with_saves", "dx_chain", "dw"}) == (mode == "train")
    for k in ("extra", "per_rank_proxy", "implied_strong_scaling_8", "frame_render", "parity", "cpu_baseline"):
        assert k not in full, k
    assert not any(k.endswith("_rays_per_s") for k in line) and "cpu_baseline" not in line and "parity" not in line


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["forward", "train"])
def test_bench_dumps_what_its_last_timed_step_returned(tmp_path, mode):
    """--dump-outputs DIR: the headline leg's last timed step as float32 .npy files (forward: C_coarse / C_fine; train step: also loss and
    one grad_<parameter> per network tensor), at most 64 MB in all.  The inputs are seeded, so a second run with the same arguments writes
    the same arrays bit for bit; --steps is the number of timed steps of the line."""
    import numpy as np

    runs = []
    for i in range(2):
        d = str(tmp_path / f"dump{i}")
        line, _ = _bench(["--mode", mode, "--steps", "3", "--warmup", "1", "--no-extra", "--no-cpu-baseline", "--dump-outputs", d], _env(), tmp_path)
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        runs.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    a, b = runs
    grads = [k for k in a if k.startswith("grad_network.")]
    assert set(a) == {"C_coarse", "C_fine"} | ({"loss", *grads} if mode == "train" else set())
    assert len(grads) == (24 if mode == "train" else 0)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["C_coarse"].shape == a["C_fine"].shape == (4096, 3)
    for k, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        assert np.array_equal(v, b[k]), k


@pytest.mark.timeout(900)
def test_bench_two_ranks_rehearsed_on_one_gpu(tmp_path):
    """The driver's N > 1 command (`python bench.py --gpus 2 ...`: this process launches the ranks itself) has never met a multi-GPU node.
    Rehearsed here with BOTH ranks on the one GPU of the box and gloo in RCCL's place (BENCH_DIST_BACKEND=gloo): the launcher, per-rank
    inputs, weak legs, the strong legs (one 4,096-ray batch split 2,048 / 2,048, the global ray 0's spacing forwarded to rank 1), the flat SUM
    all-reduce, the MAX reduction of the times, rank 0's compact line with its strong_* scalars -- the code path, not a measurement."""
    env = _env()
    env["BENCH_DIST_BACKEND"] = "gloo"
    line, full = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], env, tmp_path)
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and "rehearsal" in line
    assert line["config"]["rays_per_step_per_gpu"] == 4096 and line["value"] > 0
    for k in ("train_f32_rays_per_s", "train_bf16_rays_per_s", "strong_train_f32_rays_per_s", "strong_train_bf16_rays_per_s",
              "strong_forward_f32_rays_per_s", "strong_forward_bf16_rays_per_s", "strong_train_bf16_allreduce_ms"):
        assert line.get(k) is not None, k
    assert full["extra"]["strong_train_f32"]["rays_per_step"] == 4096
    assert "per_rank_proxy" not in full and "cpu_baseline" not in full  # N = 1 only
    assert full["parity"]["pass"] is True


def _run_ranks(n, out, extra=(), backend=None, timeout=500):
    """n ranks of tests/tools/dp_runner_rank.py under torch.distributed.run (n = 0: the plain single-process runner), fresh processes."""
    import socket

    tool = os.path.join(ROOT, "tests", "tools", "dp_runner_rank.py")
    env = _env()
    if backend:
        env["NERF_DIST_BACKEND"] = backend
    if n == 0:
        cmd = [sys.executable, tool, out, *extra]
    else:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), tool, out, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "DP-RUNNER-OK" in r.stdout
    import torch

    return torch.load(os.path.join(out, "result.pt"), weights_only=False)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("bf16,overlap", [(False, False), (True, False), (False, True), (True, True)])
def test_data_parallel_runner_single_rank_rccl_equals_plain_runner(tmp_path, bf16, overlap):
    """NeRFRunner under a launcher.  One rank over a REAL RCCL group (the collective is the identity): the data-
    parallel loop -- sharded sampler, gradients in the flat bucket, the all-reduce (one collective behind the step, or with
    overlap_allreduce=True its early part on a side stream behind the library's event), fused Adam on the views, rank 0 logging and
    checkpointing, display() through render_rows_sharded + gather_rows -- must leave bit-identical weights, losses and frames to the
    plain single-process runner (same kernels, same order of the same batches); bf16 WITH the overlap: see below."""
    import torch

    extra = ("--bf16",) if bf16 else ()
    plain = _run_ranks(0, str(tmp_path / "plain"), extra)
    dp = _run_ranks(1, str(tmp_path / "dp1"), extra + ("--force-dist",) + (("--overlap",) if overlap else ()))
    assert plain["distributed"] is False and dp["distributed"] is True and dp["ranks"] == 1 and dp["local_rays"] == 256
    assert len(dp["losses"]) == 6 and plain["losses"][0] == dp["losses"][0]
    if not (bf16 and overlap):
        assert plain["losses"] == dp["losses"]
        assert torch.equal(plain["weights"], dp["weights"])
        assert torch.equal(plain["frame"], dp["frame"])
    else:
        # bf16 weight gradients of a small batch: ONE launch for all products, or -- with the overlap's early event -- one for
        # point_layer[0..7] and one for the rest; the workgroups (= slabs) per product differ between the two, i.e. the same sums in
        # another order.  Adam turns last-bit differences into +-lr updates (tests/test_gpu_train.py: trajectory test), so from the
        # second step on the two runs are two correct trainers, not the same bits
        for a, b in zip(plain["losses"], dp["losses"]):
            assert abs(a - b) <= 3e-2 * abs(a), (plain["losses"], dp["losses"])
        d = (plain["weights"] - dp["weights"]).abs()
        assert float(d.max()) <= 2 * 1e-3 * 6 + 1e-6 and float(d.mean()) < 1e-3
        assert float((plain["frame"] - dp["frame"]).abs().max()) < 0.1
    assert len(dp["ckpts"]) == 2 and dp["ckpts"][-1].endswith("_5.pkl") and dp["images"] == 3


@pytest.mark.timeout(900)
def test_data_parallel_runner_with_the_split_train_step(tmp_path):
    """NeRFRunner(split_train=True) under a launcher: one rank over a real RCCL group must leave bit-identical weights, losses and frames to the
    plain single-process runner with the same switch (gradients in the flat bucket, the sum of the three weight-gradient sets written into
    its views), and it learns."""
    import torch

    plain = _run_ranks(0, str(tmp_path / "plain"), ("--split-train",))
    dp = _run_ranks(1, str(tmp_path / "dp1"), ("--split-train", "--force-dist"))
    assert dp["distributed"] is True and dp["ranks"] == 1
    assert plain["losses"] == dp["losses"] and torch.equal(plain["weights"], dp["weights"]) and torch.equal(plain["frame"], dp["frame"])
    assert dp["losses"][-1] < 0.6 * dp["losses"][0]
    exact = _run_ranks(0, str(tmp_path / "exact"))
    assert abs(exact["losses"][0] - plain["losses"][0]) <= 1e-5 * abs(exact["losses"][0])  # the same first step to the split arithmetic's 1e-5


@pytest.mark.timeout(900)
def test_data_parallel_runner_two_ranks_follow_the_single_process_run(tmp_path):
    """Two ranks on the box's one GPU (process group over gloo: RCCL refuses two ranks on one device; same runner code): each trains on
    its half of every 256-ray batch, the halves' gradients are SUM-all-reduced, both take the same Adam step.  The job's loss curve (the
    SUM of the ranks' losses) follows the single-process run on the same batches to summation order, the weights stay replicated (checked
    inside the ranks), the frame rendered tile-sharded over the two ranks is bit-identical to the single-process render of the same weights
    -- compared here through weights that differ only by summation order: 1e-3."""
    import torch

    plain = _run_ranks(0, str(tmp_path / "plain"))
    dp = _run_ranks(2, str(tmp_path / "dp2"), backend="gloo")
    assert dp["ranks"] == 2 and dp["local_rays"] == 128 and len(dp["ckpts"]) == 2 and dp["images"] == 3
    # step 0: the same weights on the same batch, only the summation over the two halves differs; afterwards the runs drift apart the way any
    # two correct fp32 trainers do (tests/test_gpu_train.py::test_training_trajectory_...: Adam's first updates are +-lr per element
    # whatever the gradient's size, so a 1e-6 difference is 1e-3 in the loss after ONE step) -- the curve is held to 3 %
    assert abs(plain["losses"][0] - dp["losses"][0]) <= 1e-5 * abs(plain["losses"][0]), (plain["losses"], dp["losses"])
    for a, b in zip(plain["losses"], dp["losses"]):
        assert abs(a - b) <= 3e-2 * abs(a), (plain["losses"], dp["losses"])
    assert dp["losses"][-1] < 0.6 * dp["losses"][0]
    d = (plain["weights"] - dp["weights"]).abs()
    assert float(d.max()) <= 2 * 1e-3 * 6 + 1e-6 and float(d.mean()) < 1e-3, (float(d.max()), float(d.mean()))
    assert float((plain["frame"] - dp["frame"]).abs().max()) < 0.1
