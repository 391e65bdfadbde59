"""GPU tests of per-row ranges in adaptive sweeps (ExprAdaptiveSweep::integrate_ranges,
csrc/runtime/expr_adaptive_sweep.cpp). The contract is that row r of a ranged call is, in every
field and bit for bit, row 0 of the shared-range call on [a_r, b_r] with that row alone and the
same panels and max_intervals, so the existing path is the oracle: no new numerical reference.
The exact-arithmetic integrands are also held to the host reference of
cuda_v_mpi_amd/utils/adaptive_curve.py.

The device does not report the list length of every round; what it reports of them is held to
the reference's ``lengths``: call_rounds = their count, call_evals = 15 * their sum, peak =
their maximum, and per row ``rounds`` and ``evals``, the count and 15 * the sum of its own."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_sweep_ranges_cases as rc
from cuda_v_mpi_amd import integrate_expr_adaptive_sweep
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu


def _ranged(case, rows=None, **args):
    idx = list(range(len(case.a))) if rows is None else list(rows)
    return kernels.quad_expr_sweep(case.fam.expr, case.fam.params[idx],
                                   [case.a[k] for k in idx], [case.b[k] for k in idx],
                                   **{**case.fam.args, **case.args, **args})[0]


def _one_row_shared(case, k, **args):
    """Row k alone through the shared-range path: the oracle."""
    return kernels.quad_expr_sweep(case.fam.expr, case.fam.params[[k]], case.a[k], case.b[k],
                                   **{**case.fam.args, **case.args, **args})[0]


# ------------------------------------------------------------------ 1. against the existing path
@pytest.mark.parametrize("case", rc.BITWISE, ids=repr)
def test_every_ranged_row_is_the_one_row_shared_range_call_bit_for_bit(case):
    r = _ranged(case)
    n = len(case.a)
    assert r.rows == n
    alone = [_one_row_shared(case, k) for k in range(n)]
    for k in range(n):
        assert rc.row(r, k) == rc.row(alone[k], 0), (case, k)
    live = [k for k in range(n) if case.a[k] != case.b[k]]
    assert r.call_rounds == max(a.call_rounds for a in alone)
    assert r.call_evals == sum(a.call_evals for a in alone) == int(r.evals.sum())
    assert r.peak >= max(alone[k].peak for k in live)
    assert r.peak <= sum(alone[k].peak for k in live)


def test_a_reversed_row_is_negated_and_an_empty_row_is_zero_alone():
    case = rc.MIXED
    r = _ranged(case)
    fwd = kernels.quad_expr_sweep(case.fam.expr, case.fam.params[[1]], case.b[1], case.a[1],
                                  **case.args)[0]
    assert r.value[1] < 0 and rc.row(r, 1) == rc.negated(rc.row(fwd, 0))
    assert rc.row(r, 2) == (rc.bits(0.0), rc.bits(0.0), rc.bits(0.0), rc.bits(0.0),
                            0, 0, 0, 0, 0, 0, 0, 0, 1)
    empty = _ranged(case, rows=[2], atol=1e-3)
    assert rc.bits(empty.tol[0]) == rc.bits(1e-3) and empty.converged[0]
    assert empty.call_rounds == 0 and empty.call_evals == 0 and empty.peak == 0
    # the batch without the empty row: the other rows did not notice it
    rest = _ranged(case, rows=[0, 1, 3, 4])
    for i, k in enumerate([0, 1, 3, 4]):
        assert rc.row(rest, i) == rc.row(r, k)
    assert (rest.call_rounds, rest.call_evals, rest.peak) == (r.call_rounds, r.call_evals, r.peak)


def test_one_row_caps_alone_and_the_others_do_not_notice():
    case = rc.CAPPED
    want = rc.model(case)
    assert want["capped"].tolist() == [k == rc.CAPPED_ROW for k in range(len(case.a))]
    r = _ranged(case)
    wide = _ranged(case, max_intervals=2048)
    print([rc.row(r, k) for k in range(r.rows)])
    for k in range(r.rows):
        if k == rc.CAPPED_ROW:
            assert r.capped[k] and not r.converged[k] and r.intervals[k] <= 256
            assert not wide.capped[k] and wide.converged[k]
        else:
            assert not r.capped[k] and r.converged[k]
            assert rc.row(r, k) == rc.row(wide, k)


# ------------------------------------------------------------------ 2. a shared range as arrays
@pytest.mark.parametrize("a,b", [(-1.0, 1.0), (0.5, -1.0)], ids=["forwards", "backwards"])
def test_a_shared_range_given_as_arrays_is_the_shared_range_call(a, b):
    fam, args = rc.sc.LORENTZ, dict(panels=16, max_intervals=256)
    n = len(fam.rows)
    shared = kernels.quad_expr_sweep(fam.expr, fam.params, a, b, **args)[0]
    ranged = kernels.quad_expr_sweep(fam.expr, fam.params, [a] * n, [b] * n, **args)[0]
    mixed = kernels.quad_expr_sweep(fam.expr, fam.params, a, np.full(n, b), **args)[0]
    for k in range(n):
        assert rc.row(ranged, k) == rc.row(shared, k) == rc.row(mixed, k), k
    for r in (ranged, mixed):
        assert (r.call_rounds, r.call_evals, r.peak) == (shared.call_rounds, shared.call_evals,
                                                         shared.peak)


# ------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("case", [rc.LORENTZ16, rc.LORENTZ3P, rc.COS7], ids=repr)
def test_a_ranged_row_is_bitwise_the_same_alone_in_the_batch_and_reversed(case):
    n = len(case.a)
    together = _ranged(case)
    backwards = _ranged(case, rows=range(n - 1, -1, -1))
    for k in range(n):
        alone = _ranged(case, rows=[k])
        assert rc.row(alone, 0) == rc.row(together, k) == rc.row(backwards, n - 1 - k), k
        assert alone.call_rounds == together.rounds[k]


def test_ranged_calls_are_reproducible_across_calls_and_buffer_growth():
    small, big = rc.LORENTZ16, rc.LORENTZ100
    first = [rc.row(_ranged(small), k) for k in range(5)]
    _ranged(big)   # the buffers grow, the device rows are other rows
    assert [rc.row(_ranged(small), k) for k in range(5)] == first


# ------------------------------------------------------------------ 4. the bit-exact reference
@pytest.mark.parametrize("case", rc.EXACT_CASES, ids=repr)
def test_ranged_rows_are_the_host_reference_bit_for_bit(case):
    want = rc.exact(case)
    r = kernels.quad_expr_sweep(case.expr, case.params, case.a, case.b, **case.opts)[0]
    print(case, [rc.row(r, k) for k in range(r.rows)], r.call_rounds, r.call_evals, r.peak)
    for k in range(r.rows):
        assert rc.row(r, k) == rc.row(want, k), (case, k)
    assert r.call_rounds == want["call_rounds"] == len(want["lengths"])
    assert r.call_evals == want["call_evals"] == 15 * sum(want["lengths"])
    assert r.peak == want["peak"] == max(want["lengths"])
    for k in range(r.rows):
        assert r.rounds[k] == len(want["row_lengths"][k])
        assert r.evals[k] == 15 * sum(want["row_lengths"][k])


# ------------------------------------------------------------------ 9. the model's work
@pytest.mark.parametrize("case", [rc.LORENTZ16, rc.LORENTZ3P, rc.LORENTZ100, rc.LORENTZ257,
                                  rc.COS7], ids=repr)
def test_evaluation_counts_are_the_models_within_the_projects_window(case):
    want = rc.model(case)
    r = _ranged(case)
    for k in range(r.rows):
        print(case, k, int(r.evals[k]), int(want["evals"][k]))
    for k in range(r.rows):
        assert 0.8 * want["evals"][k] <= r.evals[k] <= 1.25 * want["evals"][k], (case, k)
        assert r.converged[k] and r.evals[k] == 15 * (r.intervals[k] + r.splits[k])


# ------------------------------------------------------------------ the surfaces agree
def test_the_python_api_takes_arrays_and_agrees_bit_for_bit():
    case = rc.LORENTZ16
    r = _ranged(case)
    api = integrate_expr_adaptive_sweep(case.fam.expr, case.fam.params, case.a, case.b,
                                        backend="hip", **case.args)
    assert [rc.bits(v) for v in api.value] == [rc.bits(v) for v in r.value]
    assert api.evals.tolist() == r.evals.tolist() and api.converged.all()
    assert api.range == "finite" and api.a.tolist() == case.a
    with pytest.raises(RuntimeError, match="row 1: a = 0 and b = inf must be finite"):
        kernels.quad_expr_sweep(case.fam.expr, case.fam.params[:2], [0.0, 0.0],
                                [1.0, float("inf")])


def _clis(tmp_path, flags):
    """The native and the Python CLI's --json records for the same flags."""
    import json
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", repo, "-j8", "cli"], check=True, capture_output=True)
    out = []
    for cmd in ([exe], [sys.executable, "-m", "cuda_v_mpi_amd", "integrate"]):
        p = subprocess.run([*cmd, *flags, "--json"], cwd=repo, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr
        out.append((json.loads(p.stdout.strip().splitlines()[-1]), p.stderr))
    return out


def test_both_clis_take_a_ranges_file_and_agree_bit_for_bit(tmp_path):
    expr = "1.0/((x-p0)*(x-p0)+1e-6)"
    ends = [(-1.0, 0.0), (-0.5, 0.5), (0.3, 0.3), (1.0, 0.25)]
    path = tmp_path / "ranges.txt"
    path.write_text("# a b\n" + "".join(f"{a!r} {b!r}\n" for a, b in ends))
    from cuda_v_mpi_amd import native

    p0 = np.asarray(native().linspace_param_rows("p0=-0.5:0.7:4"), dtype=np.float64).reshape(4, 1)
    r = kernels.quad_expr_sweep(expr, p0, [e[0] for e in ends], [e[1] for e in ends], rtol=1e-9,
                                panels=16)[0]
    flags = ("--expr", expr, "--linspace", "p0=-0.5:0.7:4", "--ranges", str(path), "--row-rtol",
             "1e-9", "--panels", "16")
    for js, err in _clis(tmp_path, flags):
        assert "not converged" not in err
        assert js["value_bits"] == [rc.bits(v) for v in r.value]
        assert js["evals"] == r.evals.tolist() and js["rounds"] == r.rounds.tolist()
        assert js["a"] == [e[0] for e in ends] and js["b"] == [e[1] for e in ends]
        assert js["call_rounds"] == r.call_rounds and js["call_evals"] == r.call_evals
