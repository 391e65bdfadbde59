"""ExprAdaptive2D on the device: the (7, 15) x (7, 15) product on rectangles bisected by rounds,
held to mpmath truths and to the numpy model's work (expr_adaptive2d_cases.py derives the
value's bound; [0.8, 1.25] of the model's evaluations and one round either way are the
project's bound for a decision that falls the other way at a border)."""
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

import expr_adaptive2d_cases as ac
from cuda_v_mpi_amd import integrate_expr2d_adaptive, native
from cuda_v_mpi_amd.ops import kernels

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v: float) -> str:
    return struct.pack(">d", v).hex()


def _identities(r, panels):
    assert r.splits == r.splits_x + r.splits_y
    assert r.intervals == panels + r.splits
    assert r.evals == 225 * (r.intervals + r.splits)


def _work_matches(r, want):
    assert 0.8 * want["evals"] <= r.evals <= 1.25 * want["evals"]
    assert abs(int(r.rounds) - want["rounds"]) <= 1


def _rows(a: np.ndarray):
    """The rectangles of an n x 4 array as a set of byte strings (bitwise comparison)."""
    return {row.tobytes() for row in np.ascontiguousarray(a, dtype=np.float64)}


def _check_partition(rects: np.ndarray, box):
    """Every rectangle inside the box with positive sides, ordered by (y0, x0)."""
    ax, bx, ay, by = box
    x0, x1, y0, y1 = rects.T
    assert np.all(x1 > x0) and np.all(y1 > y0)
    assert x0.min() == ax and x1.max() == bx and y0.min() == ay and y1.max() == by
    order = np.lexsort((x0, y0))
    assert np.array_equal(order, np.arange(len(rects)))


# ------------------------------------------------------------------ 1. converged, the model's work
@pytest.mark.parametrize("run", ac.RUNS, ids=ac.run_id)
def test_converged_runs_meet_the_truth_with_the_models_work(run):
    case, rtol, (px, py) = run
    want = ac.run_model(run)
    r = kernels.quad_expr2d(case.expr, *case.box, rtol=rtol, panels=(px, py))
    print(ac.run_id(run), r.as_dict(), "model",
          {k: want[k] for k in ("evals", "rounds", "intervals", "splits_x", "splits_y", "peak")},
          "|value - truth|", abs(r.value - case.truth), "bound", ac.value_bound(r))
    # one run is honestly not converged in the model and on the device alike (ac.NOT_CONVERGED);
    # its value is still inside the bound, which takes the larger of tol and err_est
    assert want["converged"] == (run not in ac.NOT_CONVERGED)
    assert r.converged == want["converged"] and not r.capped and r.nonfinite == 0
    assert abs(r.value - case.truth) <= ac.value_bound(r)
    _identities(r, px * py)
    _work_matches(r, want)


# ------------------------------------------------------------------ 2. the axis logic
def test_a_ridge_along_y_is_split_along_x_only_and_its_transpose_along_y_only():
    args = dict(rtol=1e-10)
    r = kernels.quad_expr2d(ac.RIDGE.expr, *ac.RIDGE.box, panels=(64, 32), **args)
    t = kernels.quad_expr2d(ac.RIDGE_T.expr, *ac.RIDGE_T.box, panels=(32, 64), **args)
    print(r.as_dict(), t.as_dict())
    assert r.converged and t.converged
    assert r.splits_y == 0 and r.splits_x > 0
    assert t.splits_x == 0 and t.splits_y == r.splits_x
    assert abs(r.value - t.value) <= ac.value_bound(r)
    assert abs(r.value - ac.RIDGE.truth) <= ac.value_bound(r)
    assert abs(t.value - ac.RIDGE_T.truth) <= ac.value_bound(t)


@pytest.mark.parametrize("shape", ac.SHAPES)
def test_an_edge_singularity_in_x_is_never_split_along_y(shape):
    r = kernels.quad_expr2d(ac.EDGE.expr, *ac.EDGE.box, panels=shape)
    assert r.converged and r.splits_y == 0 and r.splits_x > 0


# ------------------------------------------------------------------ 3. the partition
def test_partition_of_the_kink_tiles_the_box():
    """|x - y| from one rectangle: 23 rounds and a list of up to 4096 (16 workgroups, splits
    and acceptances interleaved in each). All edges are dyadic, so the areas add up exactly."""
    case, args = ac.KINK, ac.KINK_ARGS
    want = ac.model(case, **args)
    cap = 1 << 14
    buf = torch.full((cap + 64, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    m = native()
    opt = m.Adapt2DOptions(rtol=args["rtol"], panels_x=1, panels_y=1, max_intervals=cap)
    r = m.ExprAdaptive2D(case.expr, 0).integrate(*case.box, opt, buf.data_ptr(), cap)
    print(r.as_dict(), "model", {k: want[k] for k in ("rounds", "intervals", "evals", "peak")})
    assert r.converged and abs(r.value - case.truth) <= ac.value_bound(r)
    _identities(r, 1)
    _work_matches(r, want)
    host = buf.cpu().numpy()
    assert np.all(host[cap:] == -7.0) and np.all(host[r.intervals:cap] == -7.0)
    rects = host[:r.intervals]
    _check_partition(rects, case.box)
    assert math.fsum((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])) == 1.0
    shared = len(_rows(rects) & _rows(want["rects"]))
    assert shared >= 0.8 * max(len(rects), len(want["rects"]))
    # the same through kernels.quad_expr2d
    r2, t = kernels.quad_expr2d(case.expr, *case.box, rtol=args["rtol"], panels=(1, 1),
                                max_intervals=cap, return_rects=True)
    assert t.shape == (r.intervals, 4) and np.array_equal(t.cpu().numpy(), rects)
    assert _bits(r2.value) == _bits(r.value)


# ------------------------------------------------------------------ 4. honest failures
def test_nan_integrand_is_accepted_and_counted():
    want = ac.model(ac.SQRT_NEG)
    r = kernels.quad_expr2d(ac.SQRT_NEG.expr, *ac.SQRT_NEG.box)
    print(r.as_dict())
    assert r.nonfinite >= 1 and math.isnan(r.value) and not r.converged and r.rounds == 1
    assert want["rounds"] == 1 and math.isnan(want["value"]) and r.nonfinite == want["nonfinite"]
    _identities(r, 64 * 64)


def test_the_disc_by_indicator_runs_to_the_cap_and_writes_nothing_past_the_buffer():
    """err of a rectangle the circle cuts is proportional to its area, so its share of the
    tolerance is never met: capped, with the value still within atol of pi."""
    case, args = ac.DISC, ac.DISC_ARGS
    want = ac.model(case, **args)
    cap = args["max_intervals"]
    m = native()
    opt = m.Adapt2DOptions(**args)
    buf = torch.full((cap + 64, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ea = m.ExprAdaptive2D(case.expr, 0)
    r = ea.integrate(*case.box, opt, buf.data_ptr(), cap)
    print(r.as_dict(), "model", {k: want[k] for k in ("rounds", "intervals", "evals", "capped")})
    assert want["capped"] and not want["converged"]
    assert r.capped and not r.converged and r.intervals <= cap
    assert abs(r.value - math.pi) <= 1e-3
    _identities(r, 16)
    _work_matches(r, want)
    host = buf.cpu().numpy()
    assert np.all(host[cap:] == -7.0)
    rects = host[:r.intervals]
    _check_partition(rects, case.box)
    assert math.fsum((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])) == 4.0
    with pytest.raises(RuntimeError, match=f"fewer than max_intervals = {cap}"):
        ea.integrate(*case.box, opt, buf.data_ptr(), cap - 1)


def test_max_depth_zero_accepts_everything_in_one_round():
    r = kernels.quad_expr2d(ac.PEAK.expr, *ac.PEAK.box, max_depth=0, panels=(17, 16))
    assert r.rounds == 1 and r.splits == 0 and r.intervals == 272 and r.forced >= 1
    assert not r.converged and r.evals == 225 * 272


# ------------------------------------------------------------------ 5. reproducible
def test_bitwise_reproducible_across_calls_objects_and_buffer_growth():
    m = native()
    case = ac.DIAGONAL
    cap = 4096
    opt = m.Adapt2DOptions(rtol=1e-6, panels_x=1, panels_y=1, max_intervals=cap)

    def run(ea, o=opt, n=cap):
        buf = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r = ea.integrate(*case.box, o, buf.data_ptr(), n)
        return (_bits(r.value), _bits(r.err_est), _bits(r.resabs), r.intervals, r.rounds,
                buf[:r.intervals].cpu().numpy())

    first = m.ExprAdaptive2D(case.expr, 0)
    one = run(first)
    assert one[3] >= 400 and one[4] >= 10
    small = first.integrate(0.0, 0.001, 0.0, 0.001, m.Adapt2DOptions(panels_x=3, panels_y=2))
    assert small.rounds >= 1 and small.intervals >= 6
    grown = m.Adapt2DOptions(rtol=1e-6, panels_x=1, panels_y=1, max_intervals=4 * cap)
    for other in (run(first), run(m.ExprAdaptive2D(case.expr, 0)), run(first, grown, 4 * cap)):
        assert other[:5] == one[:5] and np.array_equal(other[5], one[5])


def test_the_1d_sources_and_values_do_not_move_around_a_2d_object():
    m = native()
    expr = "1.0/(x*x+1e-8)"
    before = (m.expr_adapt_source(expr), m.expr_adapt_unbounded_source(expr))
    one = kernels.quad_expr(expr, -1.0, 1.0, rtol=1e-9, panels=32)
    ea = m.ExprAdaptive2D("1.0/(x*x+y*y+1e-8)", 0)
    assert ea.integrate(-1.0, 1.0, -1.0, 1.0, m.Adapt2DOptions(rtol=1e-6)).rounds >= 1
    assert (m.expr_adapt_source(expr), m.expr_adapt_unbounded_source(expr)) == before
    two = kernels.quad_expr(expr, -1.0, 1.0, rtol=1e-9, panels=32)
    assert _bits(one.value) == _bits(two.value) and one.evals == two.evals


# ------------------------------------------------------------------ 6. reversed and empty sides
def test_reversed_sides_negate_and_an_empty_side_is_zero():
    case = ac.PEAK
    args = dict(rtol=1e-8, panels=(5, 3))
    fwd, frects = kernels.quad_expr2d(case.expr, -1.0, 0.5, -0.75, 1.0, return_rects=True, **args)
    assert fwd.converged and fwd.value > 0
    for box, sign in (((0.5, -1.0, -0.75, 1.0), -1.0), ((-1.0, 0.5, 1.0, -0.75), -1.0),
                      ((0.5, -1.0, 1.0, -0.75), 1.0)):
        rev, rrects = kernels.quad_expr2d(case.expr, *box, return_rects=True, **args)
        assert _bits(rev.value) == _bits(sign * fwd.value)
        assert _bits(rev.err_est) == _bits(fwd.err_est) and rev.evals == fwd.evals
        assert rev.converged and torch.equal(rrects, frects)
    for box in ((0.25, 0.25, 0.0, 1.0), (0.0, 1.0, -0.5, -0.5)):
        z = kernels.quad_expr2d(case.expr, *box)
        assert _bits(z.value) == _bits(0.0) and z.evals == 0 and z.rounds == 0 and z.converged


# ------------------------------------------------------------------ 7. surfaces agree
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


FLAGS = ("--expr", ac.PEAK.expr, "--a", "-1", "--b", "1", "--ya", "-1", "--yb", "1",
         "--area-rtol", "1e-8", "--panels", "5", "--panels-y", "3")
JSON_KEYS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds", "intervals",
             "splits", "splits_x", "splits_y", "floor", "forced", "nonfinite", "capped",
             "device_ms")


@pytest.fixture(scope="module")
def surface_value():
    """kernels.quad_expr2d's result for FLAGS: what every other surface has to print."""
    return kernels.quad_expr2d(ac.PEAK.expr, -1.0, 1.0, -1.0, 1.0, rtol=1e-8, panels=(5, 3))


def _same(js, r):
    for k in JSON_KEYS:
        assert k in js, k
    assert _bits(js["value"]) == _bits(r.value) and js["value_bits"] == _bits(r.value)
    assert js["err_est"] == r.err_est and js["resabs"] == r.resabs and js["tol"] == r.tol
    for k in ("evals", "rounds", "intervals", "splits", "splits_x", "splits_y"):
        assert js[k] == getattr(r, k), k


def test_native_object_python_api_and_native_cli_agree_bit_for_bit(surface_value):
    r = surface_value
    m = native()
    obj = m.ExprAdaptive2D(ac.PEAK.expr, 0).integrate(
        -1.0, 1.0, -1.0, 1.0, m.Adapt2DOptions(rtol=1e-8, panels_x=5, panels_y=3))
    api = integrate_expr2d_adaptive(ac.PEAK.expr, -1.0, 1.0, -1.0, 1.0, rtol=1e-8, panels_x=5,
                                    panels_y=3, backend="hip")
    for other in (obj, api):
        assert _bits(other.value) == _bits(r.value) and _bits(other.err_est) == _bits(r.err_est)
        assert other.evals == r.evals and other.splits_x == r.splits_x and other.converged
    p = _riemann(*FLAGS, "--json")
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    _same(json.loads(p.stdout.strip().splitlines()[-1]), r)


def test_python_cli_agrees_bit_for_bit(surface_value):
    p = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *FLAGS, "--json"],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    _same(json.loads(p.stdout.strip().splitlines()[-1]), surface_value)


def test_clis_print_the_value_and_warn_when_not_converged():
    """The plain form prints the value alone; not converged: one warning line on stderr."""
    flags = ("--expr", ac.PEAK.expr, "--a", "-1", "--b", "1", "--ya", "-1", "--yb", "1",
             "--area-rtol", "1e-8", "--panels", "17", "--panels-y", "16", "--max-depth", "0")
    r = kernels.quad_expr2d(ac.PEAK.expr, -1.0, 1.0, -1.0, 1.0, rtol=1e-8, panels=(17, 16),
                            max_depth=0)
    assert not r.converged
    native_cli = _riemann(*flags)
    python_cli = subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *flags],
                                cwd=REPO, capture_output=True, text=True, timeout=300)
    for p in (native_cli, python_cli):
        assert p.returncode == 0, p.stderr
        assert len([l for l in p.stderr.splitlines() if "not converged" in l]) == 1, p.stderr
        assert _bits(float(p.stdout.strip().splitlines()[-1])) == _bits(r.value)
