"""The adaptive integrators on the device against their bit-exact reference
(cuda_v_mpi_amd/utils/adaptive_exact.py): ExprAdaptive on finite and infinite ranges,
ExprAdaptiveSweep and ExprAdaptive2D, every case of expr_adaptive_exact_cases.py once. Every
double is compared by its bits and every counter by its value: value, err_est, resabs, tol,
evals, rounds, intervals, splits (and splits_x / splits_y), floor, forced, nonfinite, converged,
capped, the sweep's per-row arrays, and the whole returned partition; behind a capped run's
buffer, the canary. There is no tolerance in this file.

What each case is there for, and that the reference takes that path, is shown without a GPU in
test_expr_adaptive_exact_cpu.py. The integrands are bit-reproducible by construction (see the
cases' docstring), so a mismatch is a kernel, its documentation or the reference misreading
the documented order: the first differing field is printed with both hex values.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_adaptive_exact_cases as ec
from cuda_v_mpi_amd import native
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

DOUBLES = ("value", "err_est", "resabs", "tol")
COUNTERS = ("evals", "rounds", "intervals", "splits", "floor", "forced", "nonfinite",
            "converged", "capped")
CANARY = -7.0
PAD = 64  # canary rows behind a buffer of max_intervals


def _hex(v) -> str:
    return float(v).hex()


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _first_difference(got: dict, want: dict, doubles, counters):
    """'' when every field agrees, else the first one that does not, with both values."""
    for key in doubles:
        g, w = np.atleast_1d(got[key]), np.atleast_1d(want[key])
        if g.shape != w.shape:
            return f"{key}: shape {g.shape} against {w.shape}"
        bad = np.flatnonzero(_bits(g) != _bits(w))
        if bad.size:
            i = int(bad[0])
            return (f"{key}[{i}] of {bad.size} differing: device {_hex(g[i])} reference "
                    f"{_hex(w[i])}")
    for key in counters:
        g, w = np.atleast_1d(got[key]).astype(np.int64), np.atleast_1d(want[key]).astype(np.int64)
        if g.shape != w.shape:
            return f"{key}: shape {g.shape} against {w.shape}"
        bad = np.flatnonzero(g != w)
        if bad.size:
            i = int(bad[0])
            return f"{key}[{i}] of {bad.size} differing: device {g[i]} reference {w[i]}"
    return ""


def _partition_difference(got: np.ndarray, want: np.ndarray):
    if got.shape != want.shape:
        return f"partition: shape {got.shape} against {want.shape}"
    bad = np.argwhere(_bits(got) != _bits(want))
    if bad.size:
        i, j = (int(v) for v in bad[0])
        return (f"partition[{i}, {j}] of {len(bad)} differing: device {_hex(got[i, j])} "
                f"reference {_hex(want[i, j])}")
    return ""


def _with_canary(integrate, columns: int, max_intervals: int, intervals_of):
    """Run into a buffer of max_intervals rows followed by PAD canary rows; returns the result,
    the rows the run filled, and whether everything behind them is untouched."""
    buf = torch.full((max_intervals + PAD, columns), CANARY, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r = integrate(buf.data_ptr(), max_intervals)
    host = buf.cpu().numpy()
    n = intervals_of(r)
    return r, host[:n].copy(), bool(np.all(host[n:] == CANARY))


# ------------------------------------------------------------------ ExprAdaptive
@pytest.mark.parametrize("case", ec.CASES_1D, ids=repr)
def test_adaptive_is_the_reference_bit_for_bit(case):
    want = ec.reference(case)
    o = dict(case.opts)
    m = native()
    if want["capped"]:
        opt = m.AdaptOptions(o.get("rtol", 1e-10), o.get("atol", 0.0), o["panels"],
                             o.get("max_depth", 60), o["max_intervals"],
                             o.get("unbounded", False))
        ea = m.ExprAdaptive(case.expr, 0)
        r, part, clean = _with_canary(
            lambda ptr, cap: ea.integrate(case.a, case.b, opt, ptr, cap), 2, o["max_intervals"],
            lambda r: r.intervals)
        assert clean, "the run wrote behind the intervals it reports"
    else:
        r, lo, hi = kernels.quad_expr(case.expr, case.a, case.b, return_intervals=True, **o)
        part = torch.stack([lo, hi], dim=1).cpu().numpy()
    got = r.as_dict()
    print(case, case.pins, {k: got[k] for k in DOUBLES + COUNTERS})
    diff = _first_difference(got, want, DOUBLES, COUNTERS)
    assert not diff, f"{case}: {diff}"
    assert got["range"] == want["range"]
    diff = _partition_difference(part, want["partition"])
    assert not diff, f"{case}: {diff}"


# ------------------------------------------------------------------ ExprAdaptiveSweep
ROW_DOUBLES = DOUBLES
ROW_COUNTERS = COUNTERS


@pytest.mark.parametrize("case", ec.SWEEP_CASES, ids=repr)
def test_sweep_is_the_reference_bit_for_bit(case):
    want = ec.reference(case)
    r, values, err_est, converged = kernels.quad_expr_sweep(
        case.expr, np.array(case.params), case.a, case.b, **case.opts)
    got = {k: np.asarray(getattr(r, k)) for k in ROW_DOUBLES + ROW_COUNTERS}
    print(case, case.pins, "call_rounds", r.call_rounds, "call_evals", r.call_evals, "peak",
          r.peak, "rounds", got["rounds"].tolist())
    diff = _first_difference(got, want, ROW_DOUBLES, ROW_COUNTERS)
    assert not diff, f"{case}: {diff}"
    assert (r.call_rounds, r.call_evals, r.peak) == (want["call_rounds"], want["call_evals"],
                                                     want["peak"])
    assert np.array_equal(_bits(values.cpu().numpy()), _bits(want["value"]))
    assert np.array_equal(_bits(err_est.cpu().numpy()), _bits(want["err_est"]))
    assert np.array_equal(converged.cpu().numpy(), want["converged"])


# ------------------------------------------------------------------ ExprAdaptive2D
COUNTERS_2D = COUNTERS + ("splits_x", "splits_y")


@pytest.mark.parametrize("case", ec.CASES_2D, ids=repr)
def test_adaptive2d_is_the_reference_bit_for_bit(case):
    want = ec.reference(case)
    o = dict(case.opts)
    m = native()
    if want["capped"]:
        px, py = o["panels"]
        opt = m.Adapt2DOptions(o.get("rtol", 1e-10), o.get("atol", 0.0), px, py,
                               o.get("max_depth", 60), o["max_intervals"])
        ea = m.ExprAdaptive2D(case.expr, 0)
        r, rects, clean = _with_canary(
            lambda ptr, cap: ea.integrate(*case.box, opt, ptr, cap), 4, o["max_intervals"],
            lambda r: r.intervals)
        assert clean, "the run wrote behind the rectangles it reports"
    else:
        r, rects = kernels.quad_expr2d(case.expr, *case.box, return_rects=True, **o)
        rects = rects.cpu().numpy()
    got = r.as_dict()
    print(case, case.pins, {k: got[k] for k in DOUBLES + COUNTERS_2D})
    diff = _first_difference(got, want, DOUBLES, COUNTERS_2D)
    assert not diff, f"{case}: {diff}"
    diff = _partition_difference(rects, want["partition"])
    assert not diff, f"{case}: {diff}"
