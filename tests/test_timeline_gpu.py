"""The per-workgroup timeline of the persistent multi-step launch (RiemannPlan::
timeline_batch, riemann.hip riemann_timeline_kernel) on the GPU: the instrumented launch
computes the plain launch's values bit for bit, every stamp cell is written and ordered, the
stamps fit inside the hipEvent span around the launch, and a plan that was instrumented once
runs its graph batches exactly as a fresh plan does."""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

SIN = dict(n=192 * 1000 + 77, rule="mid")  # a few 192-sample tiles per lane, a ragged last one
# (case id) -> (integrand, Integrator keywords, steps of the timeline batch)
CASES = {
    "sin_g5_b256": ("sin", dict(SIN, grid=5, block=256), 7),
    "sin_g17_b64": ("sin", dict(SIN, grid=17, block=64), 7),
    "sin_g100_b1024": ("sin", dict(SIN, grid=100, block=1024), 7),
    "pi4_eighth_k1": ("pi4", dict(n=10**9 // 8), 1),
    "pi4_eighth_k20": ("pi4", dict(n=10**9 // 8), 20),
    "table_o8_k20": ("table", dict(n=120_000_011), 20),
    "pi4_fp32_k20": ("pi4", dict(n=120_000_011, dtype="fp32"), 20),
}
_runs: dict = {}


def _run(case):
    """One timeline batch per case, and the plain launch's values from a second plan of the
    same grid: computed once, shared by the tests below, never modified."""
    if case in _runs:
        return _runs[case]
    from cuda_v_mpi_amd import Integrator

    name, kw, k = CASES[case]
    it = Integrator(name, slots=20, **kw)
    assert it.plan.multistep and not it.plan.close_in_launch
    t = it.timeline(k)
    slots = [it.plan.host_result(j) for j in range(k)]
    ref = Integrator(name, slots=20, **dict(kw, grid=it.plan.grid))
    assert ref.plan.grid == it.plan.grid
    ref.run_steps(k, pipeline=False, graphs=False)
    want = [ref.plan.host_result(ref.plan.host_index_of(j, False)) for j in range(k)]
    _runs[case] = (it, t, slots, want, k)
    return _runs[case]


def _bits(values):
    return [float(v).hex() for v in values]


@pytest.mark.parametrize("case", list(CASES))
def test_values_are_bitwise_the_plain_launchs(cuda, case):
    it, t, slots, want, k = _run(case)
    assert len(want) == k and all(math.isfinite(v) for v in want)
    assert _bits(slots) == _bits(want)
    assert _bits(t["values"]) == _bits(want)
    assert len(set(_bits(slots))) == 1
    assert t["steps"] == k and t["grid"] == it.plan.grid and t["block"] == it.plan.block


@pytest.mark.parametrize("case", list(CASES))
def test_every_cell_is_written_and_ordered(cuda, case):
    it, t, _, _, k = _run(case)
    g = it.plan.grid
    st, clk, hw = t["stamps"], t["shader_clock"], t["hw"]
    assert st.dtype == np.uint64 and clk.dtype == np.uint64 and hw.dtype == np.uint32
    assert st.shape == (g, k + 2) and clk.shape == (g, 2) and hw.shape == (g, 2)
    assert (st != 0).all() and (clk != 0).all() and (hw != 0xFFFFFFFF).all()  # no sentinel left
    assert (st[:, 1:] >= st[:, :-1]).all()  # every workgroup's row is non-decreasing
    assert (clk[:, 1] > clk[:, 0]).all()


@pytest.mark.parametrize("case", list(CASES))
def test_span_fits_inside_the_event_span(cuda, case):
    _, t, _, _, _ = _run(case)
    assert t["clock_khz"] > 0
    span_us = float(int(t["stamps"].max()) - int(t["stamps"].min())) / t["clock_khz"] * 1e3
    print(f"{case}: stamp span {span_us:.2f} us, event span {t['device_us']:.2f} us")
    assert span_us <= t["device_us"]  # the events bracket the launch: no tolerance


@pytest.mark.parametrize("case", list(CASES))
def test_placement(cuda, case):
    _, t, _, _, _ = _run(case)
    xcc = t["xcc"]
    assert (xcc == (t["hw"][:, 0] & 0xF)).all()
    assert ((xcc >= 0) & (xcc < 8)).all() and len(set(xcc.tolist())) <= 8


def test_repeats(cuda):
    from cuda_v_mpi_amd import Integrator

    it = Integrator("sin", slots=8, grid=17, block=64, **SIN)
    a = it.timeline(7)
    b = it.timeline(7)
    assert _bits(a["values"]) == _bits(b["values"])
    assert int(b["stamps"].min()) > int(a["stamps"].max())
    c = it.timeline(3)  # a shorter batch on the same buffers: its own row length
    assert c["stamps"].shape == (it.plan.grid, 5) and (c["stamps"] != 0).all()
    assert _bits(c["values"]) == _bits(a["values"][:3])
    assert int(c["stamps"].min()) > int(b["stamps"].max())


def test_refusals(cuda):
    from cuda_v_mpi_amd import Integrator

    kw = dict(n=10**9 // 8, slots=8)
    launch = Integrator("pi4", close="launch", **kw)
    assert launch.plan.multistep and launch.plan.close_in_launch
    with pytest.raises(RuntimeError, match="kernel-closed multi-step launch only"):
        launch.timeline(4)
    chained = Integrator("pi4", multistep=False, **kw)
    assert not chained.plan.multistep
    with pytest.raises(RuntimeError, match="not a multi-step plan"):
        chained.timeline(4)
    plain = Integrator("pi4", **kw)
    assert plain.plan.multistep and plain.plan.slots == 8
    with pytest.raises(RuntimeError, match="1 <= steps <= slots"):
        plain.timeline(9)
    with pytest.raises(RuntimeError, match="1 <= steps <= slots"):
        plain.timeline(0)
    assert len(plain.timeline(8)["values"]) == 8  # the plan is usable after a refusal


def test_the_default_path_is_unaffected(cuda):
    from cuda_v_mpi_amd import Integrator

    kw = dict(n=120_000_011, rule="mid", slots=20)
    it = Integrator("pi4", **kw)
    it.timeline(20)
    fresh = Integrator("pi4", **kw)
    for p in (it, fresh):
        p.run_steps(47, True, True)
        assert p.plan.graphs_ready, p.plan.graph_error
    assert it.plan.graph_nodes == 2  # the persistent kernel and the closing kernel
    got = [it.plan.host_result(it.plan.host_index_of(k, True)) for k in range(27, 47)]
    want = [fresh.plan.host_result(fresh.plan.host_index_of(k, True)) for k in range(27, 47)]
    assert _bits(got) == _bits(want) and len(set(_bits(got))) == 1


def test_cli_writes_a_timeline_the_report_reads(cuda, tmp_path):
    import timeline_report

    exe = os.path.join(REPO, "build", "bin", "miint")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    out = tmp_path / "tl.json"
    p = subprocess.run([exe, "bench", "--integrand", "sin", "--n", "192077", "--slots", "8",
                        "--iters", "8", "--timeline", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["timeline_file"] == str(out) and rec["multistep"]
    t = timeline_report.load(str(out))
    r = timeline_report.analyse(t)
    assert t["steps"] == 8 and t["grid"] == rec["grid"] and t["block"] == rec["block"]
    assert t["integrand"] == "sin" and t["n"] == 192077 and t["slice_of"] is None
    assert _bits(t["values"]) == _bits([rec["result"]] * 8)
    assert r["span_ticks"] == (r["start_delay_ticks"] + r["last_steps_ticks"]
                               + r["exit_segment_ticks"])
    assert r["span_us"] <= t["device_us"]
    # the in-launch close has no timeline: refused before anything runs
    q = subprocess.run([exe, "bench", "--integrand", "sin", "--n", "192077", "--slots", "8",
                        "--iters", "8", "--close", "launch", "--timeline", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert q.returncode != 0 and "kernel-closed multi-step launch only" in q.stderr


def test_cli_timeline_with_several_ranks(cuda, tmp_path):
    """The timeline batch is collective (a barrier, the bucketed all-reduce): every rank runs
    it, rank 0's is written. Two ranks sharing this GPU: the run ends, one file, the ranks'
    global step values in it."""
    import timeline_report

    exe = os.path.join(REPO, "build", "bin", "miint")
    out = tmp_path / "tl2.json"
    p = subprocess.run([exe, "bench", "--integrand", "sin", "--n", "384077", "--slots", "8",
                        "--iters", "8", "--loopback", "2", "--diagnose", "--timeline", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["gpus"] == 2 and rec["timeline_file"] == str(out)
    t = timeline_report.load(str(out))
    assert t["steps"] == 8 and t["grid"] == rec["grid"]
    assert _bits(t["values"]) == _bits([rec["result"]] * 8)  # the all-reduced values
    assert t["plain_device_us"] == rec["diag_device_us"]
