"""CPU tests of the command-line front ends (formats, argument handling, oracle dump)."""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _py(*args):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300)


def test_python_cli_riemann_cpu_format():
    p = _py("riemann", "--backend", "cpu", "--n", "1e6", "--json")
    assert p.returncode == 0, p.stderr
    l = p.stdout.strip().splitlines()
    assert l[0].endswith(" seconds") and float(l[0].split()[0]) > 0
    assert l[1].startswith("The integral of f(x) from 0.0 to 3.14159265358979 with 1000000 steps is ")
    js = json.loads(l[2])
    assert abs(js["value"] - 2.0) < 1e-11


def test_python_cli_cintegrate_parity_cpu():
    p = _py("cintegrate", "--backend", "cpu", "--parity")
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines()[1] == "final distance is:121999.800663"


def test_python_cli_table2d_cpu_matches_oracle():
    """The torch reference form of the 2-D field integral against the separable host oracle
    (sum_j v(x_j) dx)^2."""
    p = _py("table2d", "--backend", "cpu", "--grid", "300")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["grid"] == 300 and js["rel_err_vs_oracle"] < 1e-13


def test_python_cli_oracle():
    p = _py("oracle")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout)
    assert "%f" % js["trainscan_p16"] == "117642.707174"
    assert js["trainscan_p7"] == 0.0
    assert abs(js["pi4_left_n1e6_err"] - 1e-6) < 1e-9


def test_native_cli_refuses_without_gpu():
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        assert p.returncode == 1 and "HIP devices" in p.stderr


def _native(name):
    exe = os.path.join(REPO, "build", "bin", name)
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("name", ["riemann", "cintegrate", "trainscan", "miint", "miintrun"])
def test_native_cli_help_needs_no_device(name):
    p = subprocess.run([_native(name), "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("usage: " + name), p.stderr


@pytest.mark.parametrize("flag,value", [("rule", "midd"), ("dtype", "fp46"), ("div", "iee")])
def test_native_cli_rejects_misspelt_knobs(flag, value):
    # a typo must fail, not quietly run the default rule / dtype / division
    p = subprocess.run([_native("riemann"), "--device", "cpu", "--n", "1e4", f"--{flag}", value],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and f"--{flag} must be" in p.stderr


def _bench(*args, timeout=300, env=None):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args],
                          capture_output=True, text=True, timeout=timeout, env=env)


def test_bench_spawns_ranks_without_torchrun():
    """`python bench.py --gpus 2` is one command for 2 ranks (the reference's
    `mpirun -np P`, riemann.cpp:62-86): the parent spawns 2 children with RANK / LOCAL_RANK
    / WORLD_SIZE / MASTER_* set (each child asserts its env against the process group) and
    never imports torch itself, so it cannot have initialised HIP. CPU form: gloo + torch
    fp64 evaluation of each rank's slice."""
    p = _bench("--gpus", "2", "--device", "cpu", "--backend", "gloo", "--samples", "2e4",
               "--steps", "2", "--warmup", "1", "--settle-ms", "0")
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    js = json.loads(lines[0])
    assert js["n_gpus"] == 2 and js["launcher"] == "spawn"
    assert js["parent_imported_torch"] is False
    assert len(js["per_rank_ms"]) == 2 and js["per_rank_spread_ms"] >= 0
    # strong scaling (the metric's form): --samples is the TOTAL N, split over the 2 ranks
    assert js["scaling"] == "strong" and js["config"]["parallelism"] == "dp2"
    assert js["config"]["N"] == 20_000 and js["config"]["n_per_gpu"] == 10_000
    assert js["verified"] and abs(js["result"] - math.pi) < 1e-3


def test_bench_diagnostic_batch_cpu():
    """VERDICT r5 Next #2 (CPU form): a multi-rank run records, after its timed region, one
    untimed batch taken apart per rank (compute, tail = close + all-reduce + copy, host part;
    max and min over ranks) and its communicator's 8-byte all-reduce latency and allgather
    bus bandwidth. Per rank compute + tail is the batch's span. (Two CPU processes sharing
    the cores under a parallel test run time too unevenly to hold the batch against the
    timed steps; that 5 % check is the native path's, test_diagnose_batch_accounts_for_the_
    timed_batch on a GPU.)"""
    p = _bench("--gpus", "2", "--device", "cpu", "--backend", "gloo", "--samples", "8e6",
               "--steps", "3", "--warmup", "1", "--settle-ms", "0", "--full",
               "--diag-allgather-mb", "8",
               env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert p.returncode == 0, p.stderr[-3000:]
    js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    d = js["diagnostic_batch"]
    assert d["path"] == "cpu" and d["steps"] == 3
    for k in ("compute_us", "tail_us", "boundary_us", "allreduce_us", "device_us", "wall_us",
              "host_us"):
        assert len(d[k]["per_rank"]) == 2 and d[k]["max"] >= d[k]["min"], k
    assert d["compute_us"]["min"] > 0 and d["allreduce_us"]["min"] > 0
    c = d["comm"]
    assert c["transport"] == "gloo" and c["allreduce_8b_us"] > 0
    assert c["allgather_bytes"] == 8_000_000 and c["allgather_busbw_gbs"] > 0
    for r in range(2):
        assert d["device_us"]["per_rank"][r] == pytest.approx(
            d["compute_us"]["per_rank"][r] + d["tail_us"]["per_rank"][r], rel=1e-9)


def test_bench_single_gpu_record_has_no_diagnostics():
    """The diagnostic batch is a multi-rank record's: the 1-rank record is unchanged."""
    p = _bench("--device", "cpu", "--samples", "2e4", "--steps", "2", "--warmup", "1",
               "--settle-ms", "0")
    assert p.returncode == 0, p.stderr[-3000:]
    js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert "diagnostic_batch" not in js and js["verified"]


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs DIR: the timed steps' values as float64 .npy (the last step's, and every
    step of the last batch), the record's `result` among them, identical from run to run; a
    plain run carries no extras (`full` false)."""
    import numpy as np

    runs = []
    for d in ("a", "b"):
        p = _bench("--device", "cpu", "--samples", "2e4", "--steps", "3", "--warmup", "1",
                   "--settle-ms", "0", "--dump-outputs", str(tmp_path / d))
        assert p.returncode == 0, p.stderr[-3000:]
        js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert js["full"] is False and js["steps"] == 3 and js["ms_per_step"] > 0
        assert sorted(f.name for f in (tmp_path / d).iterdir()) == ["result.npy",
                                                                    "step_results.npy"]
        r, s = np.load(tmp_path / d / "result.npy"), np.load(tmp_path / d / "step_results.npy")
        assert r.dtype == s.dtype == np.float64 and r.shape == (1,) and s.shape == (3,)
        assert r[0] == s[-1] == js["result"]
        runs.append((r, s))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_bench_spawn_propagates_rank_failure():
    p = _bench("--gpus", "3", "--device", "cpu", "--backend", "gloo", "--integrand", "nope",
               "--steps", "1", "--warmup", "1")
    assert p.returncode != 0


def test_bench_rejects_world_mismatch():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2"],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WORLD_SIZE="3", RANK="0"))
    assert p.returncode == 2 and "WORLD_SIZE=3" in p.stderr


def test_scale_sweep_rows_and_efficiency(monkeypatch):
    """The GPU-count sweep's bookkeeping on a GPU-less box: counts the node cannot run get an
    explicit skipped row; efficiencies are computed against the N = 1 row."""
    from cuda_v_mpi_amd.parallel import scaling

    monkeypatch.setattr(scaling, "visible_gpus", lambda: 2)
    fake = {1: 1.0e13, 2: 1.9e13}
    monkeypatch.setattr(scaling, "run_bench", lambda n, s, w: {
        "value": fake[n], "ms_per_step": 0.075, "per_rank_spread_ms": 0.001, "scaling": "strong",
        "rccl_world": n if n > 1 else None, "config": {"graphs": True}, "verified": True,
        "baseline3_strong_1e10": {"value": fake[n] * 1.05, "ms_per_step": 0.7},
        "weak_1e9_per_gpu": {"value": fake[n] * 1.02, "ms_per_step": 0.08, "verified": True},
        "baseline5_table2d_4096": {"ms_per_integration": 0.009 / n ** 0.8}})
    monkeypatch.setattr(scaling, "run_comm", lambda n: {"allreduce_8B_us": 10.0 * n})
    rows = scaling.sweep([1, 2, 4, 8])
    assert [r["n_gpus"] for r in rows] == [1, 2, 4, 8]
    assert rows[2]["skipped"] == "only 2 devices" and rows[3]["skipped"] == "only 2 devices"
    # the row's value is the metric's own config (N = 1e9 in total: strong); weak a column
    assert rows[1]["value"] == 1.9e13
    assert rows[0]["strong_1e9_eff"] == 1.0 and abs(rows[1]["strong_1e9_eff"] - 0.95) < 1e-12
    assert rows[0]["weak_eff"] == 1.0 and abs(rows[1]["weak_eff"] - 0.95) < 1e-12
    assert rows[1]["weak_1e9_value"] == pytest.approx(1.9e13 * 1.02)
    assert abs(rows[1]["strong_eff"] - 0.95) < 1e-12
    assert abs(rows[1]["t2d_4096_us"] - 9.0 / 2 ** 0.8) < 1e-9
    assert abs(rows[1]["t2d_strong_eff"] - 2 ** 0.8 / 2) < 1e-12
    md = scaling.markdown(rows)
    assert "skipped: only 2 devices" in md and md.count("\n") == 5
    # ranks sharing GPUs: every count runs, the shared rows carry no efficiency and no
    # comm sweep (that one needs distinct devices)
    monkeypatch.setenv("MIINT_OVERSUBSCRIBE", "1")
    fake[4], fake[8] = 1.9e13, 1.9e13
    rows = scaling.sweep([1, 2, 4, 8])
    assert all("skipped" not in r for r in rows)
    assert [bool(r.get("ranks_share_gpus")) for r in rows] == [False, False, True, True]
    assert "strong_1e9_eff" not in rows[2] and "allreduce_8B_us" not in rows[3]
    assert "strong_1e9_eff" in rows[1] and "allreduce_8B_us" in rows[1]


def test_bench_driver_launch_form_json_contract():
    """The driver's exact launch form (torch.distributed.run, 127.0.0.1, a chosen port) on the
    CPU (gloo ranks): rank 0 prints ONE line carrying every field of the bench contract, with
    the whole-job value and the MAX over ranks as the step time."""
    from bench import rendezvous_port

    port = rendezvous_port()
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(REPO, "bench.py"),
                        "--gpus", "2", "--steps", "3", "--warmup", "1", "--device", "cpu",
                        "--backend", "gloo", "--samples", "3e4", "--settle-ms", "0"],
                       capture_output=True, text=True, timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    js = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int),
                 ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("scaling", str), ("vs_baseline", float),
                 ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(js[k], t), k
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in js["config"], k
    assert js["n_gpus"] == 2 and js["steps"] == 3 and js["warmup"] == 1
    assert js["launcher"] == "torchrun" and js["scaling"] == "strong"
    assert js["comm_fallback"] is None
    assert js["warmup_rearm_batch"] is False  # a GPU launch artefact: not run on the CPU path
    assert js["pre_clock_barrier"] == "host"
    assert js["metric"].startswith("Riemann subintervals/sec at N=1e9 fp64")
    assert js["ms_per_step"] == pytest.approx(max(js["per_rank_ms"]))
    assert js["value"] == pytest.approx(js["config"]["N"] * 3 / (js["ms_per_step"] * 3e-3))


def test_bench_native_ranks_build_no_torch_rccl_group():
    """One RCCL communicator per rank: with --comm native (the default) the torch process
    group is the gloo control plane and no torch nccl group is ever created; the native
    communicator is the rank's only RCCL one. CPU form, 3 ranks (gloo everywhere; the record
    states the control plane and counts torch RCCL groups)."""
    from cuda_v_mpi_amd.parallel import dist as mdist

    assert mdist.control_backend("native", "gpu") == "gloo"
    assert mdist.control_backend("torch", "gpu") == "nccl"
    assert mdist.control_backend("native", "cpu") == "gloo"
    p = _bench("--gpus", "3", "--device", "cpu", "--samples", "3e4", "--steps", "2",
               "--warmup", "1", "--settle-ms", "0")
    assert p.returncode == 0, p.stderr[-3000:]
    js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert js["n_gpus"] == 3 and js["control_plane"] == "gloo"
    assert js["torch_nccl_groups"] == 0
    assert js["verified"] and js["headline_verified"]


def test_bench_verification_bounds():
    """The record's pass/fail rules: 4/(1+x^2) truncation per rule in closed form, fp32 at
    2h, and a wrong value fails."""
    sys.path.insert(0, REPO)
    import bench

    h = 1e-9
    assert bench.result_ok("pi4", "left", "fp64", 10**9, 1.000000082740371e-09)
    assert bench.result_ok("pi4", "left", "fp64", 10**10, 1.000000082740371e-10)
    assert bench.result_ok("pi4", "left", "fp64", 10**6, 9.999998336063243e-07)  # h - h^2/6
    assert not bench.result_ok("pi4", "left", "fp64", 10**9, 1.2e-9)
    assert not bench.result_ok("pi4", "left", "fp64", 10**9, 0.0)
    assert bench.result_ok("pi4", "mid", "fp64", 10**9, 4e-16)
    assert not bench.result_ok("pi4", "mid", "fp64", 10**9, 1e-12)
    assert bench.result_ok("pi4", "left", "fp32", 10**9, 1.0195799760026603e-09)
    assert not bench.result_ok("pi4", "left", "fp32", 10**9, 3 * h)
    assert not bench.result_ok("pi4", "left", "fp64", 10**9, float("nan"))


def test_bench_eight_rank_rehearsal():
    """The driver's 8-GPU scaling run, rehearsed on the CPU: 8 spawned rank processes, the gloo
    control plane (no torch RCCL group), one time per rank, MAX over ranks, the metric's
    fixed total N split 8 ways (strong), every rank's result verified."""
    p = _bench("--gpus", "8", "--device", "cpu", "--samples", "8e4", "--steps", "2",
               "--warmup", "1", "--settle-ms", "0", timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert js["n_gpus"] == 8 and len(js["per_rank_ms"]) == 8
    assert js["control_plane"] == "gloo" and js["torch_nccl_groups"] == 0
    assert js["config"]["N"] == 80_000 and js["config"]["parallelism"] == "dp8"
    assert js["config"]["n_per_gpu"] == 10_000 and js["scaling"] == "strong"
    assert js["ms_per_step"] == pytest.approx(max(js["per_rank_ms"]))
    assert js["verified"]


def test_bench_multi_rank_record_is_the_metric_config():
    """VERDICT r4 Next #1: at G > 1 the top-level record IS the metric's config, N = 1e9 in
    total split over the ranks (riemann.cpp:10,71-73), not a weak N = G x 1e9 figure printed
    under the N = 1e9 metric string. CPU form (gloo, torch fp64 evaluation): 2 ranks, 5e8
    samples each, the left-rule truncation of N = 1e9 (h - h^2/6) checked to 1e-13."""
    p = _bench("--gpus", "2", "--device", "cpu", "--steps", "1", "--warmup", "1",
               "--settle-ms", "0", timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    js = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert js["metric"] == "Riemann subintervals/sec at N=1e9 fp64; |error| vs analytic π"
    assert js["scaling"] == "strong" and js["n_gpus"] == 2
    assert js["config"]["N"] == 10**9 and js["config"]["n_per_gpu"] == 5 * 10**8
    assert js["config"]["global_batch"] == 10**9
    assert js["verified"] and abs(js["abs_err"] - (1e-9 - 1e-18 / 6)) <= 1e-13
    assert js["value"] == pytest.approx(10**9 / (js["ms_per_step"] * 1e-3))
    # the CPU path runs no native plan: no batches to launch, none claimed
    assert js["config"]["batch_launch"] == "none" and not js["config"]["multistep"]
