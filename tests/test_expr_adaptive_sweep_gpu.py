"""GPU tests of adaptive sweeps (ExprAdaptiveSweep, csrc/runtime/expr_adaptive_sweep.cpp): every
row against its closed-form truth and against the numpy model of the same rule
(cuda_v_mpi_amd/utils/adaptive_quad.py, adaptive_sweep_model), and a row against itself alone.

The value's bound. A converged row is held to

    |value - truth| <= max(tol, err_est) + 48 * 2^-52 * resabs

The first term is what the rule promises, the second is rounding. With u = 2^-53 and R_i the
rule's integral of |f| over interval i of the row (resabs is their sum), from the row kernel's
own order of summation (one wave per row: lane l chains elements l, l + 64, ... of the row's
segment, then a 64-lane butterfly):
  * K_i: f to 2 u relative, the pair sum u, eight chained fma u each, the product with hw u:
    12 u R_i (as in test_expr_adaptive_gpu.py);
  * the round's sum of the row's accepted K: a lane's chain holds at most ceil(L / 64) elements,
    L the row's longest list. The longest list a case here reaches is 998 (cos(2000 x) from one
    panel; the model's ``peak_row``): 16 elements, 15 additions, then the butterfly's 6: at
    most 21 u R of the round, and the rounds' R add up to R;
  * the rounds, added in order onto S_acc: at most max_depth + 1 = 61 additions, 61 u R;
  * the truth, rounded to a double: u |truth| <= u R.
Together 95 u R = 47.5 * 2^-52 R; the tests use 48. (ExprAdaptive's 77 has two block
reductions where a row has one chain and one butterfly.) What f makes of a rounded argument
(cos(2000 x) turns a node's u into 2000 u of f) is not rounding of the sums and is not in the
slack: the cosine rows run at rtol = 1e-9, where it stays an order of magnitude inside tol."""
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
import expr_adaptive_sweep_cases as sc
from cuda_v_mpi_amd import integrate_expr_adaptive_sweep, native
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = ("value", "err_est", "resabs", "tol")
COUNTS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite", "capped",
          "converged")


def _bits(v) -> str:
    return struct.pack(">d", float(v)).hex()


def _row(r, k: int) -> tuple:
    """Everything the result says about row k: the doubles as bits, then the counters."""
    return (tuple(_bits(getattr(r, f)[k]) for f in F64)
            + tuple(int(getattr(r, f)[k]) for f in COUNTS))


def _sweep(fam, rows=None, **args):
    params = fam.params if rows is None else fam.params[list(rows)]
    return kernels.quad_expr_sweep(fam.expr, params, fam.a, fam.b, **{**fam.args, **args})[0]


def _check_against_truth_and_model(fam, r, want, panels):
    """The assertions of tests 1 and 2, per row."""
    k_rows = len(fam.rows)
    assert r.rows == k_rows
    for k in range(k_rows):
        err = abs(r.value[k] - fam.truths[k])
        print(fam, fam.rows[k], _row(r, k), "model evals", want["evals"][k], "rounds",
              want["rounds"][k], "|value - truth|", err, "bound", sc.value_bound(r, k))
    for k in range(k_rows):
        assert r.converged[k] and not r.capped[k] and r.nonfinite[k] == 0, k
        assert abs(r.value[k] - fam.truths[k]) <= sc.value_bound(r, k), k
        assert r.intervals[k] == panels + r.splits[k], k
        assert r.evals[k] == 15 * (r.intervals[k] + r.splits[k]), k
        assert 0.8 * want["evals"][k] <= r.evals[k] <= 1.25 * want["evals"][k], k
    assert r.call_evals == int(r.evals.sum())
    assert r.call_rounds == int(r.rounds.max())


# ------------------------------------------------------------------ 1. truth and model, per row
@pytest.mark.parametrize("panels", [16, 3])
@pytest.mark.parametrize("fam", [sc.LORENTZ, sc.KINK, sc.STEP], ids=repr)
def test_every_row_meets_its_truth_with_the_models_work(fam, panels):
    """One sweep per family; 3 panels put the rows' boundaries inside waves."""
    want = sc.model(fam, panels=panels)
    r = _sweep(fam, panels=panels)
    _check_against_truth_and_model(fam, r, want, panels)


def test_cosine_rows_from_one_panel():
    want = sc.model(sc.COS)
    r = _sweep(sc.COS)
    _check_against_truth_and_model(sc.COS, r, want, 1)
    assert r.peak >= 600


# ------------------------------------------------------------------ 2. segments across workgroups
@pytest.mark.parametrize("fam,args,panels", [
    (sc.COS7, sc.COS7_ARGS, 1),
    (sc.LORENTZ100, dict(panels=3), 3),
    (sc.LORENTZ3, dict(panels=257), 257),
], ids=["cos7", "lorentz100x3", "lorentz3x257"])
def test_segments_across_workgroups(fam, args, panels):
    """Several ~1000-interval segments beside 1-interval ones (splits and acceptances
    interleave across workgroup and row boundaries); 100 rows of 3; 3 rows of 257."""
    want = sc.model(fam, **args)
    r = _sweep(fam, **args)
    _check_against_truth_and_model(fam, r, want, panels)


# ------------------------------------------------------------------ 3. row independence
def test_a_row_is_bitwise_the_same_alone_reversed_and_in_the_batch():
    fam, args = sc.LORENTZ, dict(panels=16, max_intervals=256)
    n = len(fam.rows)
    together = _sweep(fam, **args)
    backwards = _sweep(fam, rows=range(n - 1, -1, -1), **args)
    for k in range(n):
        alone = _sweep(fam, rows=[k], **args)
        assert _row(alone, 0) == _row(together, k) == _row(backwards, n - 1 - k), k
        assert alone.call_rounds == together.rounds[k]
    fam, args = sc.COS7, sc.COS7_ARGS
    together = _sweep(fam, **args)
    alone = {}
    for k, row in enumerate(fam.rows):
        if row not in alone:
            alone[row] = _row(_sweep(fam, rows=[k], **args), 0)
        assert alone[row] == _row(together, k), k


# ------------------------------------------------------------------ 4. NaN containment
def test_a_nan_row_stays_in_its_row():
    fam, args = sc.SQRT_SHIFT, dict(panels=16)
    want = sc.model(fam, **args)
    assert list(want["nonfinite"]) == sc.SQRT_SHIFT_NONFINITE and list(want["rounds"][1:]) == [1, 1]
    r = _sweep(fam, **args)
    print([_row(r, k) for k in range(3)])
    for k in (1, 2):
        assert math.isnan(r.value[k]) and r.nonfinite[k] >= 1 and not r.converged[k]
    assert r.nonfinite[0] == 0 and r.converged[0]
    assert abs(r.value[0] - fam.truths[0]) <= sc.value_bound(r, 0)
    assert _row(_sweep(fam, rows=[0], **args), 0) == _row(r, 0)
    # a NaN row between two finite ones
    fam = sc.LORENTZ_NAN
    r = _sweep(fam, **args)
    assert math.isnan(r.value[1]) and r.nonfinite[1] >= 1 and not r.converged[1]
    for k in (0, 2):
        assert r.converged[k] and math.isfinite(r.value[k])
        assert _row(_sweep(fam, rows=[k], **args), 0) == _row(r, k)


# ------------------------------------------------------------------ 5. per-row cap
def test_a_capped_row_stops_alone():
    fam = sc.LORENTZ
    want = sc.model(fam, panels=16)
    assert list(want["intervals"]) == sc.LORENTZ_MODEL_INTERVALS
    wide = _sweep(fam, panels=16, max_intervals=256)
    r = _sweep(fam, panels=16, max_intervals=32)
    print([_row(r, k) for k in range(5)])
    for k, n in enumerate(sc.LORENTZ_MODEL_INTERVALS):
        if n > 32:
            assert r.capped[k] and not r.converged[k] and math.isfinite(r.value[k])
            assert r.intervals[k] <= 32
            assert r.evals[k] == 15 * (r.intervals[k] + r.splits[k])
        else:
            assert _row(r, k) == _row(wide, k)
    assert r.peak <= 5 * 32


# ------------------------------------------------------------------ 6. early rows leave
def test_rows_that_finish_early_leave_the_rounds():
    fam = sc.STEP.with_rows("step_mixed", [(0.5,), (1.0 / 3.0,), (0.5,), (0.25,)])
    r = kernels.quad_expr_sweep(fam.expr, fam.params, fam.a, fam.b, panels=16)[0]
    print([_row(r, k) for k in range(4)], r.call_rounds, r.call_evals, r.peak)
    assert r.call_rounds == int(r.rounds.max()) == int(r.rounds[1]) and r.rounds[1] >= 45
    for k in (0, 2, 3):   # the step sits on a panel edge: one round
        assert r.rounds[k] == 1 and r.evals[k] == 15 * 16 and r.converged[k]
    assert r.call_evals == int(r.evals.sum()) and r.peak == 4 * 16


# ------------------------------------------------------------------ 7. against ExprAdaptive
def test_one_row_without_parameters_against_expr_adaptive():
    case = ac.RESONANCE
    args = dict(rtol=1e-10, panels=16, max_intervals=4096)
    want = ac.model(case, rtol=1e-10, panels=16)
    one = kernels.quad_expr(case.expr, case.a, case.b, **args)
    r = kernels.quad_expr_sweep(case.expr, [[]], case.a, case.b, max_total=4096, **args)[0]
    print(one.as_dict(), _row(r, 0))
    assert r.rows == 1 and r.converged[0] and one.converged
    assert abs(one.value - case.truth) <= ac.value_bound(one)
    assert abs(r.value[0] - case.truth) <= sc.value_bound(r, 0)
    for evals in (one.evals, int(r.evals[0])):
        assert 0.8 * want["evals"] <= evals <= 1.25 * want["evals"]


# ------------------------------------------------------------------ 8. reproducible
def test_bitwise_reproducible_across_calls_buffer_growth_and_objects():
    m = native()
    fam = sc.LORENTZ
    opt = m.AdaptSweepOptions(panels=16, max_intervals=256, max_total=2048)

    def run(es):
        r = es.integrate(fam.params, fam.a, fam.b, opt)
        return [_row(r, k) for k in range(r.rows)] + [r.call_rounds, r.call_evals, r.peak]

    first = m.ExprAdaptiveSweep(fam.expr, 2, 0)
    one = run(first)
    big = first.integrate(sc.LORENTZ100.params, fam.a, fam.b,
                          m.AdaptSweepOptions(panels=3, max_total=1 << 16))   # the buffers grow
    small = first.integrate(fam.params[:1], fam.a, fam.b, m.AdaptSweepOptions(panels=3))
    assert big.rows == 100 and small.rows == 1
    assert run(first) == one
    assert run(m.ExprAdaptiveSweep(fam.expr, 2, 0)) == one


# ------------------------------------------------------------------ 9. a > b, a == b, no rows
def test_reversed_range_negates_and_empty_cases_are_empty():
    fam, args = sc.LORENTZ, dict(panels=16, rtol=1e-8)
    fwd = kernels.quad_expr_sweep(fam.expr, fam.params, -1.0, 0.5, **args)[0]
    rev = kernels.quad_expr_sweep(fam.expr, fam.params, 0.5, -1.0, **args)[0]
    for k in range(len(fam.rows)):
        a, b = _row(fwd, k), _row(rev, k)
        assert b[0] == _bits(-fwd.value[k]) and a[1:] == b[1:]
    z, values, errs, conv = kernels.quad_expr_sweep(fam.expr, fam.params, 0.25, 0.25)
    assert z.rows == 5 and all(_bits(v) == _bits(0.0) for v in z.value)
    assert z.converged.all() and z.call_evals == 0 and z.call_rounds == 0 and not z.evals.any()
    assert values.shape == (5,) and conv.all()
    e, values, errs, conv = kernels.quad_expr_sweep(fam.expr, [], -1.0, 1.0)
    assert e.rows == 0 and e.call_evals == 0 and values.numel() == 0 and conv.numel() == 0


# ------------------------------------------------------------------ 10. surfaces agree
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


SURFACE_EXPR = "1.0/((x-p0)*(x-p0)+1e-6)"
FLAGS = ("--expr", SURFACE_EXPR, "--a", "-1", "--b", "1", "--linspace", "p0=-0.5:0.7:4",
         "--row-rtol", "1e-9", "--panels", "16")
JSON_KEYS = ("value", "value_bits", "err_est", "resabs", "tol", "converged", "evals", "rounds",
             "intervals", "splits", "floor", "forced", "nonfinite", "capped", "rows",
             "call_rounds", "call_evals", "peak", "device_ms")


@pytest.fixture(scope="module")
def surface():
    """kernels.quad_expr_sweep's result for FLAGS: what every other surface has to print."""
    p0 = native().linspace_param_rows("p0=-0.5:0.7:4")
    params = np.asarray(p0, dtype=np.float64).reshape(4, 1)
    return params, kernels.quad_expr_sweep(SURFACE_EXPR, params, -1.0, 1.0, rtol=1e-9, panels=16)


def test_python_api_and_native_cli_agree_bit_for_bit(surface):
    params, (r, values, errs, conv) = surface
    assert [_bits(v) for v in values.cpu().numpy()] == [_bits(v) for v in r.value]
    assert [_bits(v) for v in errs.cpu().numpy()] == [_bits(v) for v in r.err_est]
    assert conv.cpu().numpy().tolist() == r.converged.tolist() and values.is_cuda
    api = integrate_expr_adaptive_sweep(SURFACE_EXPR, params, -1.0, 1.0, rtol=1e-9, panels=16,
                                        backend="hip")
    assert [_bits(v) for v in api.value] == [_bits(v) for v in r.value]
    assert api.evals.tolist() == r.evals.tolist() and api.converged.all()
    p = _riemann(*FLAGS, "--json")
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    for k in JSON_KEYS:
        assert k in js, k
    assert js["rows"] == 4 and js["value_bits"] == [_bits(v) for v in r.value]
    assert [_bits(v) for v in js["value"]] == [_bits(v) for v in r.value]
    assert js["evals"] == r.evals.tolist() and js["err_est"] == r.err_est.tolist()
    assert js["call_rounds"] == r.call_rounds and js["call_evals"] == r.call_evals


def test_python_cli_agrees_bit_for_bit(surface):
    params, (r, *_) = surface
    p = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *FLAGS, "--json"],
                       cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    for k in JSON_KEYS:
        assert k in js, k
    assert js["value_bits"] == [_bits(v) for v in r.value]
    assert js["rounds"] == r.rounds.tolist()


def test_native_cli_prints_the_rows_and_warns_once_when_a_row_did_not_converge():
    expr = "1.0/sqrt(fabs(x-p0))"   # p0 = 0: an endpoint singularity that 1e-13 does not reach
    flags = ("--expr", expr, "--a", "0", "--b", "1", "--linspace", "p0=0:-1:2", "--row-rtol",
             "1e-13", "--panels", "16")
    params = np.array([[0.0], [-1.0]])
    r = kernels.quad_expr_sweep(expr, params, 0.0, 1.0, rtol=1e-13, panels=16)[0]
    p = _riemann(*flags)
    assert p.returncode == 0, p.stderr
    warnings = [l for l in p.stderr.splitlines() if "not converged" in l]
    assert len(warnings) == 1 and "1 of 2 rows" in warnings[0], p.stderr
    assert not r.converged[0] and r.converged[1]
    printed = [float(l.split()[-1]) for l in p.stdout.strip().splitlines()[-2:]]
    assert [_bits(v) for v in printed] == [_bits(v) for v in r.value]
