"""GPU tests of the adaptive integrators on infinite and half-infinite ranges (the unbounded eval
kernels of csrc/runtime/expr_adaptive.cpp and expr_adaptive_sweep.cpp): the device against
closed-form truths and against the numpy model of the same rule, which evaluates f at the
device's abscissae (adapt_range_map).

The value's bound is derived in expr_adaptive_inf_cases.py:

    |value - truth| <= max(tol, err_est) + (S + 2) * 2^-52 * resabs + 3 * 2^-53 * C

with S = 96 (ExprAdaptive) or 48 (a sweep's row) from the finite tests' order of summation, 2
for the division by t * t and the pair sum of (-inf, inf), and C the integral of
(|x - end| + |x|) |f'(x)|, the integrand's conditioning against the three roundings of the
abscissa. Every test prints measured / bound."""
from __future__ import annotations

import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_cases as ac
import expr_adaptive_inf_cases as ic
from cuda_v_mpi_amd import integrate_expr_adaptive, integrate_expr_adaptive_sweep, native
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import adaptive_quad as aq

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
MAX_IV = ic.MAX_INTERVALS
F64 = ("value", "err_est", "resabs", "tol")
COUNTS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite", "capped",
          "converged")


def _bits(v) -> str:
    return struct.pack(">d", float(v)).hex()


def _all(r) -> tuple:
    return tuple(_bits(getattr(r, f)) for f in F64) + tuple(int(getattr(r, f)) for f in COUNTS)


def _row(r, k: int) -> tuple:
    return (tuple(_bits(getattr(r, f)[k]) for f in F64)
            + tuple(int(getattr(r, f)[k]) for f in COUNTS))


def _identities(r, panels):
    assert r.intervals == panels + r.splits
    assert r.evals == 15 * (r.intervals + r.splits)


def _quad(case, a=None, b=None, **args):
    args.setdefault("max_intervals", MAX_IV)
    return kernels.quad_expr(case.expr, case.a if a is None else a, case.b if b is None else b,
                             unbounded=True, **args)


# ------------------------------------------------------------------ 1. the table, both tolerances
@pytest.mark.parametrize("panels", [ic.FEW_PANELS, ic.PANELS])
@pytest.mark.parametrize("rtol", ic.RTOLS)
@pytest.mark.parametrize("case", ic.TABLE, ids=repr)
def test_table_case_meets_its_truth_with_the_models_work(case, rtol, panels):
    want = ic.model(case, rtol=rtol, panels=panels)
    r = _quad(case, rtol=rtol, panels=panels)
    err, bound = abs(r.value - case.truth), ic.value_bound(r, case)
    print(case, rtol, panels, r.as_dict(), "model evals", want["evals"], "rounds", want["rounds"],
          "|value - truth|", err, "bound", bound, "measured/bound", err / bound)
    assert r.converged and not r.capped and r.nonfinite == 0
    assert err <= bound
    _identities(r, panels)
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]
    assert abs(int(r.rounds) - want["rounds"]) <= 1
    assert r.range == aq.range_kind(case.a, case.b)


# ------------------------------------------------------------------ 2. kinds, swapped forms, a == b
@pytest.mark.parametrize("case", [ic.EXP_UP, ic.EXP_LOW, ic.GAUSS, ic.GAUSS_M2], ids=repr)
def test_swapped_ends_negate_and_the_range_is_reported(case):
    fwd = _quad(case, panels=16)
    rev = _quad(case, a=case.b, b=case.a, panels=16)
    assert fwd.range == rev.range == aq.range_kind(case.a, case.b)
    assert _bits(rev.value) == _bits(-fwd.value) and _all(rev)[1:] == _all(fwd)[1:]
    assert fwd.converged and abs(fwd.value - case.truth) <= ic.value_bound(fwd, case)


def test_equal_ends_are_zero_with_no_launch_and_finite_ends_report_finite():
    for a in (INF, -INF, 0.25):
        z = kernels.quad_expr("exp(-x*x)", a, a, unbounded=True)
        assert _bits(z.value) == _bits(0.0) and z.evals == 0 and z.rounds == 0 and z.converged
        assert z.range == "finite"
    assert kernels.quad_expr("exp(-x*x)", 0.0, 1.0, panels=16).range == "finite"


# ------------------------------------------------------------------ 3. reproducible; the finite path
def test_bitwise_reproducible_and_the_finite_path_is_untouched():
    """One object: a finite call, unbounded calls of all three kinds (the second module loads at
    the first), a call that grows the buffers, and the finite call again."""
    m = native()
    case = ac.RESONANCE
    ea = m.ExprAdaptive(case.expr, 0)
    fin_opt = m.AdaptOptions(rtol=1e-9, panels=32, max_intervals=4096)
    before = ea.integrate(case.a, case.b, fin_opt)
    flagged = ea.integrate(case.a, case.b, m.AdaptOptions(rtol=1e-9, panels=32,
                                                          max_intervals=4096, unbounded=True))
    assert _all(flagged) == _all(before) and flagged.range == "finite"
    opt = m.AdaptOptions(rtol=1e-10, panels=16, max_intervals=4096, unbounded=True)
    first = {ends: _all(ea.integrate(*ends, opt))
             for ends in ((-INF, INF), (0.5, INF), (-INF, 0.5))}
    grown = ea.integrate(-INF, INF, m.AdaptOptions(rtol=1e-10, panels=8192, max_intervals=MAX_IV,
                                                   unbounded=True))
    assert grown.converged and grown.intervals >= 8192
    for ends, want in first.items():
        assert _all(ea.integrate(*ends, opt)) == want, ends
    other = m.ExprAdaptive(case.expr, 0)
    assert _all(other.integrate(-INF, INF, opt)) == first[(-INF, INF)]
    assert _all(ea.integrate(case.a, case.b, fin_opt)) == _all(before)
    fresh = m.ExprAdaptive(case.expr, 0).integrate(case.a, case.b, fin_opt)
    assert _all(fresh) == _all(before)
    # the whole axis is the two halves: each kind against the closed form of its own range
    e = math.sqrt(1e-8)
    both, upper, lower = (first[k] for k in ((-INF, INF), (0.5, INF), (-INF, 0.5)))
    value = lambda t: struct.unpack(">d", bytes.fromhex(t[0]))[0]   # noqa: E731
    assert abs(value(both) - math.pi / e) <= 1e-9 * math.pi / e
    assert abs(value(upper) - (math.pi / 2 - math.atan(0.5 / e)) / e) <= 1e-9 * math.pi / e
    assert abs(value(upper) + value(lower) - value(both)) <= 1e-9 * math.pi / e


# ------------------------------------------------------------------ 4. the partition in t
@pytest.mark.parametrize("case,rtol", [(ic.GAUSS_50, 1e-10), (ic.RESONANCE, 1e-10),
                                       (ic.RESONANCE, 1e-13)],
                         ids=["gauss_at_50", "resonance_at_3", "resonance_at_3_into_the_noise"])
def test_partition_in_t_from_one_panel(case, rtol):
    """From one panel: the partition of [0, 1] in t, edge by edge, with a canary behind the
    caller's buffer. At rtol = 1e-10 both cases converge on a few dozen intervals. Several
    workgroups' worth come from the resonance at 1e-13: x = q near 3 carries a rounding of 3 u,
    which the width 1e-3 of the line turns into 3000 u of f, above the floor of 50 ulps, so the
    rule bisects noise until the cap (the model: 3068 intervals, a list of up to 1844, capped).
    That run is held to the partition, the counters and the bound, not to the model's work."""
    m = native()
    cap = 4096
    noise = rtol < 1e-12
    want = ic.model(case, rtol=rtol, panels=1, max_intervals=cap)
    opt = m.AdaptOptions(rtol=rtol, panels=1, max_intervals=cap, unbounded=True)
    buf = torch.full((cap + 64, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r = m.ExprAdaptive(case.expr, 0).integrate(case.a, case.b, opt, buf.data_ptr(), cap)
    host = buf.cpu().numpy()
    err, bound = abs(r.value - case.truth), ic.value_bound(r, case)
    print(case, rtol, r.as_dict(), "model",
          {k: want[k] for k in ("rounds", "intervals", "evals", "peak", "capped")},
          "|value - truth|", err, "bound", bound)
    assert r.intervals <= cap
    assert np.all(host[cap:] == -7.0) and np.all(host[r.intervals:cap] == -7.0)
    lo, hi = host[:r.intervals, 0], host[:r.intervals, 1]
    assert lo[0] == 0.0 and hi[-1] == 1.0 and np.array_equal(hi[:-1], lo[1:])
    assert np.all(hi > lo) and math.fsum(hi - lo) == 1.0       # dyadic edges: exact
    _identities(r, 1)
    assert err <= bound
    if noise:
        assert r.intervals >= 3 * 256 and want["intervals"] >= 3 * 256
    else:
        assert r.converged and not r.capped
        assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]
        assert abs(int(r.rounds) - want["rounds"]) <= 1
        shared = np.intersect1d(lo, want["lo"]).size
        assert shared >= 0.8 * max(lo.size, want["lo"].size)
    # the same through kernels.quad_expr, and in x
    r2, tlo, thi = kernels.quad_expr(case.expr, case.a, case.b, rtol=rtol, panels=1,
                                     max_intervals=cap, return_intervals=True, unbounded=True)
    assert _all(r2) == _all(r) and np.array_equal(tlo.cpu().numpy(), lo)
    assert np.array_equal(thi.cpu().numpy(), hi)
    q = aq.t_to_x(case.a, case.b, lo)
    assert q[0] == INF and np.all(np.diff(q) < 0)


# ------------------------------------------------------------------ 5. honest failures, the cap
def test_a_diverging_integral_reports_that_it_did_not_converge():
    want = ic.model(ic.DIVERGES, rtol=1e-10, panels=16)
    r = _quad(ic.DIVERGES, rtol=1e-10, panels=16)
    print(r.as_dict(), "model", {k: want[k] for k in COUNTS}, want["err_est"])
    assert not r.converged and not r.capped and r.nonfinite == 0
    assert r.rounds == 61 and 2 <= r.forced <= 3 and 1.0 <= r.err_est <= 3.0
    _identities(r, 16)
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]


def test_a_singularity_at_the_finite_end_reports_nonfinite_and_its_split_converges():
    want = ic.model(ic.END_SINGULAR, rtol=1e-6, panels=16)
    r = _quad(ic.END_SINGULAR, rtol=1e-6, panels=16)
    print(r.as_dict(), "model", {k: want[k] for k in COUNTS})
    assert not r.converged and r.nonfinite >= 1 and not r.capped
    _identities(r, 16)
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]
    # the advice: a finite call on [0, 1] and the tail (1, inf), each within its own bound
    head = kernels.quad_expr(ic.END_SINGULAR.expr, 0.0, 1.0, rtol=1e-8, panels=16,
                             max_intervals=MAX_IV)
    tail = _quad(ic.SPLIT_TAIL, rtol=1e-8, panels=16)
    e_head, e_tail = abs(head.value - ic.SPLIT_HEAD_TRUTH), abs(tail.value - ic.SPLIT_TAIL.truth)
    print("head", head.as_dict(), e_head, ac.value_bound(head), "tail", tail.as_dict(), e_tail,
          ic.value_bound(tail, ic.SPLIT_TAIL))
    assert head.converged and head.range == "finite" and e_head <= ac.value_bound(head)
    assert tail.converged and tail.range == "upper"
    assert e_tail <= ic.value_bound(tail, ic.SPLIT_TAIL)


def test_cap_just_above_the_panels_stops_the_run():
    r = _quad(ic.POWER, rtol=1e-10, panels=64, max_intervals=66)
    print(r.as_dict())
    assert r.capped and not r.converged and math.isfinite(r.value) and r.intervals <= 66
    _identities(r, 64)
    assert abs(r.value - 2.0) <= 10 * r.err_est


# ------------------------------------------------------------------ 6. sweeps
def _sweep(fam, rows=None, a=None, b=None, **args):
    params = fam.params if rows is None else fam.params[list(rows)]
    return kernels.quad_expr_sweep(fam.expr, params, fam.a if a is None else a,
                                   fam.b if b is None else b, unbounded=True, **args)[0]


@pytest.mark.parametrize("fam", ic.FAMILIES, ids=repr)
def test_every_row_of_a_sweep_meets_its_truth_with_the_models_work(fam):
    want = ic.sweep_model(fam, panels=16)
    r = _sweep(fam, panels=16)
    assert r.rows == len(fam.rows) and r.range == aq.range_kind(fam.a, fam.b)
    worst = 0.0
    for k in range(r.rows):
        err, bound = abs(r.value[k] - fam.truths[k]), ic.row_bound(r, k, fam)
        worst = max(worst, err / bound)
        if r.rows <= 8:
            print(fam, fam.rows[k], _row(r, k), "model evals", want["evals"][k], "err", err,
                  "bound", bound, "measured/bound", err / bound)
        assert r.converged[k] and not r.capped[k] and r.nonfinite[k] == 0, k
        assert err <= bound, k
        assert r.intervals[k] == 16 + r.splits[k], k
        assert r.evals[k] == 15 * (r.intervals[k] + r.splits[k]), k
        assert 0.8 * want["evals"][k] <= r.evals[k] <= 1.25 * want["evals"][k], k
        assert abs(int(r.rounds[k]) - int(want["rounds"][k])) <= 1, k
    print(fam, "worst measured/bound", worst)
    assert r.call_evals == int(r.evals.sum()) and r.call_rounds == int(r.rounds.max())


def test_a_sweeps_row_is_bitwise_the_same_alone_reversed_and_in_the_batch():
    fam = ic.GAUSS_WIDTHS
    n = len(fam.rows)
    together = _sweep(fam, panels=16)
    backwards = _sweep(fam, rows=range(n - 1, -1, -1), panels=16)
    for k in range(n):
        alone = _sweep(fam, rows=[k], panels=16)
        assert _row(alone, 0) == _row(together, k) == _row(backwards, n - 1 - k), k
    rev = _sweep(fam, a=fam.b, b=fam.a, panels=16)
    for k in range(n):
        assert _row(rev, k)[0] == _bits(-together.value[k]) and _row(rev, k)[1:] == _row(together, k)[1:]
    z = kernels.quad_expr_sweep(fam.expr, fam.params, INF, INF, unbounded=True)[0]
    assert z.rows == n and not z.value.any() and z.converged.all() and z.call_evals == 0


def test_a_diverging_row_stops_alone_while_its_neighbours_converge():
    """Row 1 is 1.0 / (x + p0) on (0, inf); rows 0 and 2 are exp(-x)."""
    want = aq.adaptive_sweep_model(ic.mixed_f, ic.MIXED_ROWS, 0.0, INF, panels=16, unbounded=True)
    r = kernels.quad_expr_sweep(ic.MIXED_EXPR, ic.MIXED_ROWS, 0.0, INF, panels=16,
                                unbounded=True)[0]
    print([_row(r, k) for k in range(3)], "model rounds", want["rounds"])
    assert not r.converged[1] and r.rounds[1] == 61 and r.forced[1] >= 2 and r.err_est[1] >= 1.0
    assert not want["converged"][1]
    for k in (0, 2):
        assert r.converged[k] and r.rounds[k] == want["rounds"][k] == 1
        assert abs(r.value[k] - 1.0) <= r.tol[k]
        alone = kernels.quad_expr_sweep(ic.MIXED_EXPR, ic.MIXED_ROWS[[k]], 0.0, INF, panels=16,
                                        unbounded=True)[0]
        assert _row(alone, 0) == _row(r, k)
    assert r.call_rounds == 61


def test_one_row_without_parameters_against_expr_adaptive():
    case = ic.RESONANCE
    args = dict(rtol=1e-10, panels=16, max_intervals=4096)
    want = ic.model(case, rtol=1e-10, panels=16)
    one = kernels.quad_expr(case.expr, case.a, case.b, unbounded=True, **args)
    r = kernels.quad_expr_sweep(case.expr, [[]], case.a, case.b, max_total=4096, unbounded=True,
                                **args)[0]
    print(one.as_dict(), _row(r, 0))
    assert r.rows == 1 and r.converged[0] and one.converged and r.range == one.range == "both"
    assert abs(one.value - case.truth) <= ic.value_bound(one, case)
    assert abs(r.value[0] - case.truth) <= ic.value_bound(
        dict(tol=r.tol[0], err_est=r.err_est[0], resabs=r.resabs[0]), case, ic.SWEEP_SLACK_UNITS)
    for evals in (one.evals, int(r.evals[0])):
        assert 0.8 * want["evals"] <= evals <= 1.25 * want["evals"]


def test_a_sweep_object_runs_finite_and_unbounded_calls_bitwise_reproducibly():
    m = native()
    fam = ic.RESONANCES
    params = fam.params[:5]
    es = m.ExprAdaptiveSweep(fam.expr, 2, 0)
    fin = m.AdaptSweepOptions(panels=16, max_intervals=512)
    unb = m.AdaptSweepOptions(panels=16, max_intervals=512, unbounded=True)

    def rows(r):
        return [_row(r, k) for k in range(r.rows)] + [r.call_rounds, r.call_evals, r.peak]

    before = rows(es.integrate(params, -6.0, 6.0, fin))
    assert rows(es.integrate(params, -6.0, 6.0, unb)) == before
    one = rows(es.integrate(params, -INF, INF, unb))
    big = es.integrate(fam.params, -INF, INF, m.AdaptSweepOptions(panels=16, unbounded=True))
    assert big.rows == 100 and big.converged.all()                 # the buffers grew
    assert rows(es.integrate(params, -INF, INF, unb)) == one
    assert rows(m.ExprAdaptiveSweep(fam.expr, 2, 0).integrate(params, -INF, INF, unb)) == one
    assert rows(es.integrate(params, -6.0, 6.0, fin)) == before


# ------------------------------------------------------------------ 7. the four surfaces
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def _py(*args):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300)


def test_the_four_surfaces_agree_bit_for_bit():
    m = native()
    expr = "exp(-x*x)"
    opt = m.AdaptOptions(rtol=1e-10, unbounded=True)
    nat = m.ExprAdaptive(expr, 0).integrate(-INF, INF, opt)
    ker = kernels.quad_expr(expr, -INF, INF, rtol=1e-10, unbounded=True)
    api = integrate_expr_adaptive(expr, -INF, INF, rtol=1e-10)
    assert _all(nat) == _all(ker) and _bits(api.value) == _bits(nat.value)
    assert api.range == ker.range == nat.range == "both" and api.converged
    assert abs(nat.value - math.sqrt(math.pi)) <= ic.value_bound(nat, ic.GAUSS)
    p = _riemann("--expr", expr, "--a", "-inf", "--b", "inf", "--rtol", "1e-10", "--json")
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["value_bits"] == _bits(nat.value) and js["converged"] is True
    assert js["range"] == "both" and js["evals"] == nat.evals and js["a"] is None
    p = _riemann("--expr", expr, "--a", "-inf", "--b", "inf", "--rtol", "1e-10")
    assert p.returncode == 0 and _bits(float(p.stdout.strip())) == _bits(nat.value)
    p = _py("--expr", expr, "--a", "-inf", "--b", "inf", "--rtol", "1e-10")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["value_bits"] == _bits(nat.value) and js["converged"] is True
    assert js["range"] == "both" and js["a"] == "-inf" and js["b"] == "inf"
    half = kernels.quad_expr("exp(-x)", 0.0, INF, rtol=1e-10, unbounded=True)
    p = _py("--expr", "exp(-x)", "--a", "0", "--b", "inf", "--rtol", "1e-10")
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["value_bits"] == _bits(half.value) and js["converged"] and js["range"] == "upper"
    assert abs(half.value - 1.0) <= ic.value_bound(half, ic.EXP_UP)


def test_the_sweeps_surfaces_agree_bit_for_bit():
    expr = "1.0/((x-p0)*(x-p0)+1e-4)"
    p0 = native().linspace_param_rows("p0=-2:3:4")
    params = np.asarray(p0, dtype=np.float64).reshape(4, 1)
    r = kernels.quad_expr_sweep(expr, params, -INF, INF, rtol=1e-10, unbounded=True)[0]
    api = integrate_expr_adaptive_sweep(expr, params, -INF, INF, rtol=1e-10)
    bits = [_bits(v) for v in r.value]
    assert [_bits(v) for v in api.value] == bits and api.converged.all() and api.range == "both"
    assert np.all(np.abs(r.value - math.pi / math.sqrt(1e-4)) <= 2 * r.tol)
    flags = ("--expr", expr, "--a", "-inf", "--b", "+inf", "--linspace", "p0=-2:3:4",
             "--row-rtol", "1e-10", "--json")
    p = _riemann(*flags)
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["value_bits"] == bits and js["range"] == "both" and all(js["converged"])
    p = _py(*flags)
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["value_bits"] == bits and js["range"] == "both" and js["not_converged"] == 0


def test_every_surface_says_that_and_why_a_run_did_not_converge():
    r = kernels.quad_expr("1.0/x", 1.0, INF, rtol=1e-10, panels=16, unbounded=True)
    api = integrate_expr_adaptive("1.0/x", 1.0, INF, rtol=1e-10, panels=16)
    assert not r.converged and not api.converged and api.forced == r.forced >= 2
    flags = ("--expr", "1.0/x", "--a", "1", "--b", "inf", "--rtol", "1e-10", "--panels", "16")
    for p in (_riemann(*flags, "--json"), _py(*flags)):
        assert p.returncode == 0, p.stderr
        warn = [l for l in p.stderr.splitlines() if "not converged" in l]
        assert len(warn) == 1 and f"forced {r.forced}" in warn[0] and "nonfinite 0" in warn[0]
        js = json.loads(p.stdout.strip().splitlines()[-1])
        assert js["converged"] is False and js["forced"] == r.forced
        assert js["value_bits"] == _bits(r.value)
    flags = ("--expr", ic.END_SINGULAR.expr, "--a", "0", "--b", "inf", "--rtol", "1e-6",
             "--panels", "16", "--max-intervals", str(MAX_IV))
    r = _quad(ic.END_SINGULAR, rtol=1e-6, panels=16)
    for p in (_riemann(*flags, "--json"), _py(*flags)):
        assert p.returncode == 0, p.stderr
        warn = [l for l in p.stderr.splitlines() if "not converged" in l]
        assert len(warn) == 1 and f"nonfinite {r.nonfinite}" in warn[0] and r.nonfinite >= 1
        js = json.loads(p.stdout.strip().splitlines()[-1])
        assert js["converged"] is False and js["nonfinite"] == r.nonfinite
