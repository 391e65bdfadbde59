"""GPU tests of the running integral to a tolerance (ExprAdaptiveCurve,
csrc/runtime/expr_adaptive_sweep.cpp): every cell against the one-row sweep call on its range
with atol_c (bit for bit: the existing path is the oracle), the per-point arrays against
miint_acurve_prefix's order on the host (cuda_v_mpi_amd/utils/adaptive_curve.py,
curve_prefix_exact) bit for bit, and the points against closed forms.

The value's bound. Point j is held to

    |F_j - truth| <= max(tol_j, err_est_j) + 98 * 2^-52 * resabs_j

The first term is what the rule promises (err_est_j, the sum of the cells' estimates, held to
tol_j, the sum of their tolerances), the second is rounding; expr_sweep_ranges_cases.py derives
the 98 from the documented orders for grids of at most 100 cells: 94 u for a cell's value as a
sweep row forms it, M u for the chain of the prefix, u for the truth, u = 2^-53."""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import expr_sweep_ranges_cases as rc
from cuda_v_mpi_amd import integrate_expr_curve
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils import adaptive_curve as acv
from cuda_v_mpi_amd.utils.adaptive_quad import adaptive_curve_model

pytestmark = pytest.mark.gpu

POINT_F64 = ("value", "err_est", "tol", "resabs")


def _curve(expr, x, **args):
    return kernels.quad_expr_curve(expr, x, **args)[0]


def _bits(v) -> list:
    return [rc.bits(t) for t in np.asarray(v, dtype=np.float64)]


def _check_prefix(r):
    """The per-point arrays are miint_acurve_prefix's order over the cells' own numbers."""
    for key in POINT_F64:
        assert _bits(getattr(r, key)) == _bits(acv.curve_prefix_exact(getattr(r.cells, key))), key
    assert r.converged.tolist() == (acv.curve_unconverged_exact(r.cells.converged) == 0).tolist()
    assert rc.bits(r.total) == rc.bits(r.value[-1])
    assert rc.bits(r.total_err_est) == rc.bits(r.err_est[-1])
    assert rc.bits(r.total_tol) == rc.bits(r.tol[-1])
    assert rc.bits(r.total_resabs) == rc.bits(r.resabs[-1])
    assert r.unconverged == int((~r.cells.converged).sum())


# ------------------------------------------------------------------ 5. the cells
@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_every_cell_is_the_one_row_call_with_its_share_of_atol(descending):
    expr, args = "exp(-x*x)", dict(rtol=1e-10, panels=4, max_intervals=256)
    atol = 1e-12
    x = rc.prefix_grid(40)[::-1].copy() if descending else rc.prefix_grid(40)
    r = _curve(expr, x, atol=atol, **args)
    whole = abs(float(x[-1]) - float(x[0]))
    tail = 0
    for c in range(40):
        atol_c = (atol * abs(float(x[c + 1]) - float(x[c]))) / whole
        assert rc.bits(r.atol_cell[c]) == rc.bits(atol_c)
        one = kernels.quad_expr_sweep(expr, [[]], float(x[c]), float(x[c + 1]), atol=atol_c,
                                      **args)[0]
        assert rc.row(r.cells, c) == rc.row(one, 0), c
        tail += rc.bits(r.cells.tol[c]) == rc.bits(atol_c)
    assert 0 < tail < 40   # cells where atol_c decides, and cells where rtol |I_c| does
    assert r.call_rounds == int(r.cells.rounds.max())
    assert r.call_evals == int(r.cells.evals.sum())
    _check_prefix(r)


# ------------------------------------------------------------------ 6. the prefix
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 513])
def test_the_points_are_the_prefix_kernels_order_bit_for_bit(m):
    """per flips from 1 to 2 between 256 and 257 (trailing threads own empty runs); 513 cells:
    per = 3 and 171 threads are busy. cos(5 x) changes sign, so the sums cancel and their order
    shows in the bits."""
    r = _curve("cos(5.0*x)", rc.prefix_grid(m), rtol=1e-9, atol=1e-12, panels=2,
               max_intervals=64)
    assert r.points == m + 1 and r.cells.rows == m
    assert all(rc.bits(getattr(r, key)[0]) == rc.bits(0.0) for key in POINT_F64)
    assert r.converged[0]
    _check_prefix(r)
    if m == 513:   # the run bounds matter: another per gives other bits
        other = acv.curve_prefix_exact(r.cells.value, per_of=lambda n: 4)
        assert _bits(other) != _bits(r.value)


def test_the_device_tensors_are_the_results_arrays():
    r, values, errs, tols, conv = kernels.quad_expr_curve("cos(5.0*x)", rc.prefix_grid(7),
                                                          panels=2)
    assert values.is_cuda and values.shape == (8,)
    assert _bits(values.cpu().numpy()) == _bits(r.value)
    assert _bits(errs.cpu().numpy()) == _bits(r.err_est)
    assert _bits(tols.cpu().numpy()) == _bits(r.tol)
    assert conv.cpu().numpy().tolist() == r.converged.tolist()
    api = integrate_expr_curve("cos(5.0*x)", rc.prefix_grid(7), panels=2, backend="hip")
    assert _bits(api.value) == _bits(r.value) and api.cells["evals"].tolist() == \
        r.cells.evals.tolist()


# ------------------------------------------------------------------ 7. the truth
def _check_truth(r, truths):
    for j, t in enumerate(truths):
        print(j, float(r.x[j]), float(r.value[j]), abs(r.value[j] - t), rc.curve_bound(r, j),
              bool(r.converged[j]))
    assert r.cells.rows <= rc.CURVE_MAX_CELLS_FOR_SLACK
    for j, t in enumerate(truths):
        assert abs(r.value[j] - t) <= rc.curve_bound(r, j), j


def test_erf_on_a_grid_of_100_cells():
    r = _curve("exp(-x*x)", rc.ERF_GRID)
    _check_truth(r, rc.ERF_TRUTH)
    assert r.converged.all() and r.call_rounds <= 3
    # relatively accurate at every point, not on the scale of the total
    assert np.all(r.tol[1:] <= 1.0000001e-10 * r.resabs[1:])


def test_an_endpoint_singularity_in_cell_zero():
    """1/sqrt(x) from 0: cell 0 goes to the depth limit, the others take one round."""
    r = _curve("1.0/sqrt(x)", rc.RSQRT_GRID, panels=16)
    _check_truth(r, [2.0 * math.sqrt(float(v)) for v in rc.RSQRT_GRID])
    print(r.cells.rounds.tolist(), r.cells.intervals.tolist())
    assert r.cells.rounds[0] >= 50 and (r.cells.rounds[1:] <= 2).all()
    assert r.call_rounds == int(r.cells.rounds[0])


def test_a_kink_inside_a_cell():
    r = _curve("fabs(x-0.3)", rc.KINK_GRID, panels=4)
    _check_truth(r, [rc.kink_truth(float(v)) for v in rc.KINK_GRID])
    assert r.converged.all() and r.cells.rounds[1] > r.cells.rounds[0] == r.cells.rounds[2] == 1


def test_a_descending_grid_is_the_ascending_cells_negated():
    """The cells of the reversed grid are the ascending grid's cells in reverse order with their
    values negated and nothing else changed; the points are the prefix of those, so the last one
    is minus the ascending cells summed from the far end."""
    x = rc.prefix_grid(40)
    args = dict(rtol=1e-10, atol=1e-9, panels=4, max_intervals=256)
    up, down = _curve("exp(-x*x)", x, **args), _curve("exp(-x*x)", x[::-1].copy(), **args)
    for c in range(40):
        assert rc.row(down.cells, c) == rc.negated(rc.row(up.cells, 39 - c)), c
    assert (down.value[1:] < 0).all()
    _check_prefix(down)
    assert rc.bits(down.value[0]) == rc.bits(0.0)   # the start is +0 on either grid
    assert _bits(down.value[1:]) == _bits(-acv.curve_prefix_exact(up.cells.value[::-1])[1:])
    assert _bits(down.err_est) == _bits(acv.curve_prefix_exact(up.cells.err_est[::-1]))


# ------------------------------------------------------------------ 8. a cell that is not finite
@pytest.mark.parametrize("expr,x,bad", [
    ("1.0/(x-0.5)", [0.0, 0.125, 0.25, 0.75, 1.0], 2),      # the centre of cell 2 is the pole
    ("sqrt(x-0.5)", [1.0, 0.875, 0.75, 0.625, 0.375, 0.25], 3),   # cell 3 reaches below 0.5
], ids=["pole", "sqrt"])
def test_a_non_finite_cell_marks_the_points_from_it_on_and_none_before(expr, x, bad):
    """With atol = 0 a cell does not see the whole width, and with M <= 256 the prefix is one
    chain, so the points before the bad cell are bitwise those of the grid cut off there."""
    args = dict(panels=1, max_intervals=64)
    r = _curve(expr, x, **args)
    cut = _curve(expr, x[:bad + 1], **args)
    assert r.cells.nonfinite[bad] >= 1 and not r.cells.converged[bad]
    assert r.converged.tolist() == [j <= bad for j in range(len(x))]
    assert cut.converged.all()
    for key in POINT_F64:
        assert _bits(getattr(r, key)[:bad + 1]) == _bits(getattr(cut, key)), key
    for c in range(bad):
        assert rc.row(r.cells, c) == rc.row(cut.cells, c)
    assert r.unconverged >= 1 and not math.isfinite(r.value[bad + 1])
    _check_prefix(r)


def test_a_capped_cell_marks_the_points_from_it_on():
    r = _curve("1.0/sqrt(x)", rc.RSQRT_GRID[::-1].copy(), panels=16, max_intervals=32)
    print(r.cells.capped.tolist(), r.converged.tolist())
    assert r.cells.capped.tolist() == [False] * 7 + [True]
    assert r.converged.tolist() == [True] * 8 + [False]
    _check_prefix(r)


# ------------------------------------------------------------------ 9. the model's work
@pytest.mark.parametrize("expr,f,x,args", [
    ("exp(-x*x)", lambda t: np.exp(-t * t), rc.ERF_GRID, {}),
    ("1.0/sqrt(x)", lambda t: 1.0 / np.sqrt(t), rc.RSQRT_GRID, dict(panels=16)),
], ids=["erf", "rsqrt"])
def test_evaluation_counts_are_the_models_within_the_projects_window(expr, f, x, args):
    want = adaptive_curve_model(f, x, **args)
    r = _curve(expr, x, **args)
    for c in range(r.cells.rows):
        print(c, int(r.cells.evals[c]), int(want["cells"]["evals"][c]))
        assert (0.8 * want["cells"]["evals"][c] <= r.cells.evals[c]
                <= 1.25 * want["cells"]["evals"][c]), c
    assert np.allclose(r.value, want["value"], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ the surfaces agree
def test_both_clis_print_the_curve_and_agree_bit_for_bit(tmp_path):
    import json
    import subprocess

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", repo, "-j8", "cli"], check=True, capture_output=True)
    grid =0.0 + ((3.0 - 0.0) * np.arange(11.0)) / 10.0   # the CLIs' own formula
    grid[-1] = 3.0
    r = _curve("exp(-x*x)", grid, rtol=1e-9, atol=1e-12)
    at = tmp_path / "grid.txt"
    at.write_text("".join(f"{v!r}\n" for v in grid.tolist()))
    for how in (("--a", "0", "--b", "3", "--points", "10"), ("--at", str(at))):
        flags = ("--expr", "exp(-x*x)", "--curve-rtol", "1e-9", "--curve-atol", "1e-12", *how)
        for cmd in ([exe], [sys.executable, "-m", "cuda_v_mpi_amd", "integrate"]):
            if cmd[0] != exe and how[0] == "--at":
                continue   # one Python start is enough: the grid's two sources meet in the native CLI
            p = subprocess.run([*cmd, *flags, "--json"], cwd=repo, capture_output=True, text=True,
                               timeout=300)
            assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
            js = json.loads(p.stdout.strip().splitlines()[-1])
            assert js["value_bits"] == [rc.bits(v) for v in r.value]
            assert js["x"] == grid.tolist() and js["points"] == 11
            assert js["err_est"] == r.err_est.tolist() and js["tol"] == r.tol.tolist()
            assert js["converged"] == [True] * 11
            assert js["cells"]["evals"] == r.cells.evals.tolist()
            assert js["call_rounds"] == r.call_rounds and js["call_evals"] == r.call_evals
    p = subprocess.run([exe, "--expr", "exp(-x*x)", "--curve-rtol", "1e-9", "--curve-atol",
                        "1e-12", "--a", "0", "--b", "3", "--points", "10"], capture_output=True,
                       text=True, timeout=120)
    lines = [l.split() for l in p.stdout.strip().splitlines()]
    assert len(lines) == 11 and [rc.bits(float(l[1])) for l in lines] == _bits(r.value)
    p = subprocess.run([exe, "--expr", "sqrt(x-0.5)", "--curve-rtol", "1e-9", "--a", "1", "--b",
                        "0", "--points", "4", "--panels", "1"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "not converged: 2 of 4 cells, the first one cell 2" in p.stderr
