"""ExprAdaptiveRegion on the device: double integrals of f(x, y) for y between two curves, the
region mapped onto [ax, bx] x [0, 1] and ExprAdaptive2D's rounds on the mapped integrand, held to
mpmath truths and to the numpy model's work (expr_region_cases.py derives the value's bound;
[0.8, 1.25] of the model's evaluations and one round either way are the project's bound for a
decision that falls the other way at a border)."""
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
import expr_region_cases as rc
from cuda_v_mpi_amd import AdaptiveRegionResult, integrate_expr2d_region, native
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.utils.adaptive_quad2d import region_corners

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("evals", "rounds", "intervals", "splits_x", "splits_y", "peak")


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


def _check_partition(rects: np.ndarray, xrange):
    """Every rectangle inside [ax, bx] x [0, 1] with positive sides, ordered by (v0, x0)."""
    x0, x1, v0, v1 = rects.T
    assert np.all(x1 > x0) and np.all(v1 > v0)
    assert (x0.min(), x1.max(), v0.min(), v1.max()) == (*xrange, 0.0, 1.0)
    assert np.array_equal(np.lexsort((x0, v0)), np.arange(len(rects)))


def _quad(case, xrange=None, **args):
    return kernels.quad_expr2d_region(case.expr, *(xrange or case.xrange), case.y_lo, case.y_hi,
                                      **args)


# ------------------------------------------------------------------ 1. converged, the model's work
@pytest.mark.parametrize("run", rc.RUNS, ids=rc.run_id)
def test_converged_runs_meet_the_truth_with_the_models_work(run):
    case, (px, py) = run
    want = rc.run_model(run)
    r = _quad(case, panels=(px, py), **case.args)
    print(rc.run_id(run), r.as_dict(), "model", {k: want[k] for k in FIELDS},
          "|value - truth|", abs(r.value - case.truth), "bound", rc.value_bound(r))
    assert want["converged"]
    assert r.converged and not r.capped and r.nonfinite == 0
    assert abs(r.value - case.truth) <= rc.value_bound(r)
    _identities(r, px * py)
    _work_matches(r, want)


# ------------------------------------------------------------------ 2. signs
def test_crossing_limits_and_reversed_ends_negate_exactly():
    c = rc.CROSSING
    left = _quad(c, (-1.0, 0.0), rtol=1e-10, panels=(4, 4))     # h < g: counted negatively
    right = _quad(c, (0.0, 1.0), rtol=1e-10, panels=(4, 4))
    assert left.converged and right.converged and abs(right.value - 0.5) <= 1e-15
    assert _bits(left.value) == _bits(-right.value) and _bits(left.resabs) == _bits(right.resabs)
    assert left.resabs > 0.49
    for case in (rc.PARABOLA, rc.DISC_GAUSS):
        args = dict(rtol=1e-10, panels=(3, 5), return_rects=True)
        (fwd, frects), (rev, rrects) = _quad(case, **args), _quad(case, case.xrange[::-1], **args)
        assert fwd.converged and rev.converged and fwd.value > 0
        assert _bits(rev.value) == _bits(-fwd.value) and _bits(rev.err_est) == _bits(fwd.err_est)
        assert rev.evals == fwd.evals and torch.equal(rrects, frects)
    z = _quad(rc.PARABOLA, (0.25, 0.25))
    assert _bits(z.value) == _bits(0.0) and z.evals == 0 and z.rounds == 0 and z.converged


# ------------------------------------------------------------------ 3. the partition
def test_partition_of_the_disc_tiles_the_mapped_rectangle():
    """The unit disc from one rectangle: 46 rounds towards the two ends of [-1, 1], where
    sqrt(1 - x^2) has its branch points. All edges are dyadic, so the areas add up exactly."""
    case = rc.DISC
    want = rc.model(case, rtol=1e-10, panels_x=1, panels_y=1)
    cap = 1024
    buf = torch.full((cap + 64, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    m = native()
    opt = m.Adapt2DOptions(rtol=1e-10, panels_x=1, panels_y=1, max_intervals=cap)
    r = m.ExprAdaptiveRegion(*case.triple, 0).integrate(*case.xrange, opt, buf.data_ptr(), cap)
    print(r.as_dict(), "model", {k: want[k] for k in FIELDS})
    assert r.converged and abs(r.value - case.truth) <= rc.value_bound(r)
    _identities(r, 1)
    _work_matches(r, want)
    host = buf.cpu().numpy()
    assert np.all(host[cap:] == -7.0) and np.all(host[r.intervals:cap] == -7.0)   # the canary
    rects = host[:r.intervals]
    _check_partition(rects, case.xrange)
    assert math.fsum((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])) == 2.0
    assert _rows(rects) == _rows(want["rects"]) and np.array_equal(rects, want["rects"])
    # the corners in (x, y) lie on or inside the circle, up to the limits' rounding
    xy = region_corners(rects, case.g, case.h)
    assert xy.shape == (r.intervals, 4, 2)
    assert np.all(xy[:, :, 0] ** 2 + xy[:, :, 1] ** 2 <= 1.0 + 4 * rc.U)
    # the same through kernels.quad_expr2d_region
    r2, t = _quad(case, rtol=1e-10, panels=(1, 1), max_intervals=cap, return_rects=True)
    assert t.shape == (r.intervals, 4) and np.array_equal(t.cpu().numpy(), rects)
    assert _bits(r2.value) == _bits(r.value)


# ------------------------------------------------------------------ 4. honest failures
def test_a_limit_that_is_not_finite_is_counted_as_nonfinite():
    """sqrt(1 - x^2) is NaN outside [-1, 1]: those rectangles are accepted and counted."""
    case = rc.DISC
    want = rc.model(case, (-2.0, 2.0))
    r = _quad(case, (-2.0, 2.0))
    print(r.as_dict())
    assert r.nonfinite >= 1 and math.isnan(r.value) and not r.converged and not r.capped
    assert want["nonfinite"] >= 1 and math.isnan(want["value"]) and not want["converged"]
    assert 0.8 * want["nonfinite"] <= r.nonfinite <= 1.25 * want["nonfinite"]
    _identities(r, 64 * 64)


def test_the_disc_runs_to_a_small_cap_and_writes_nothing_past_it():
    case = rc.DISC
    cap = 64
    want = rc.model(case, rtol=1e-10, panels_x=4, panels_y=4, max_intervals=cap)
    m = native()
    opt = m.Adapt2DOptions(rtol=1e-10, panels_x=4, panels_y=4, max_intervals=cap)
    buf = torch.full((cap + 64, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ea = m.ExprAdaptiveRegion(*case.triple, 0)
    r = ea.integrate(*case.xrange, opt, buf.data_ptr(), cap)
    print(r.as_dict(), "model", {k: want[k] for k in ("rounds", "intervals", "evals", "capped")})
    assert want["capped"] and not want["converged"]
    assert r.capped and not r.converged and r.intervals <= cap and r.nonfinite == 0
    assert abs(r.value - math.pi) <= 1e-3
    _identities(r, 16)
    _work_matches(r, want)
    host = buf.cpu().numpy()
    assert np.all(host[cap:] == -7.0) and np.all(host[r.intervals:cap] == -7.0)
    rects = host[:r.intervals]
    _check_partition(rects, case.xrange)
    assert math.fsum((rects[:, 1] - rects[:, 0]) * (rects[:, 3] - rects[:, 2])) == 2.0
    with pytest.raises(RuntimeError, match=f"fewer than max_intervals = {cap}"):
        ea.integrate(*case.xrange, opt, buf.data_ptr(), cap - 1)


# ------------------------------------------------------------------ 5. reproducible
def test_bitwise_reproducible_across_calls_objects_and_buffer_growth():
    m = native()
    case = rc.DISC_GAUSS
    cap = 1024
    opt = m.Adapt2DOptions(rtol=1e-10, panels_x=1, panels_y=1, max_intervals=cap)

    def run(ea, o=opt, n=cap):
        buf = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        r = ea.integrate(*case.xrange, o, buf.data_ptr(), n)
        return (_bits(r.value), _bits(r.err_est), _bits(r.resabs), r.intervals, r.rounds,
                buf[:r.intervals].cpu().numpy())

    first = m.ExprAdaptiveRegion(*case.triple, 0)
    one = run(first)
    assert one[3] >= 80 and one[4] >= 40
    small = first.integrate(0.0, 0.001, m.Adapt2DOptions(panels_x=3, panels_y=2))
    assert small.rounds >= 1 and small.intervals >= 6
    grown = m.Adapt2DOptions(rtol=1e-10, panels_x=1, panels_y=1, max_intervals=8 * cap)
    for other in (run(first), run(m.ExprAdaptiveRegion(*case.triple, 0)),
                  run(first, grown, 8 * cap)):
        assert other[:5] == one[:5] and np.array_equal(other[5], one[5])


def test_a_rectangle_result_does_not_move_around_region_calls():
    """ExprAdaptive2D on the same device, before and after region objects were built and run."""
    m = native()
    case = ac.PEAK
    opt = m.Adapt2DOptions(rtol=1e-8, panels_x=5, panels_y=3)

    def rectangle():
        r = m.ExprAdaptive2D(case.expr, 0).integrate(*case.box, opt)
        return (_bits(r.value), _bits(r.err_est), _bits(r.resabs), _bits(r.tol), r.evals,
                r.rounds, r.intervals, r.splits_x, r.splits_y)

    source = m.expr_adapt2d_source(case.expr)
    before = rectangle()
    cached = kernels.quad_expr2d(case.expr, *case.box, rtol=1e-8, panels=(5, 3))
    for region in (rc.PEAK_IN_DISC, rc.PARABOLA):
        assert _quad(region, rtol=1e-8, panels=(5, 3)).converged
    assert rectangle() == before and m.expr_adapt2d_source(case.expr) == source
    again = kernels.quad_expr2d(case.expr, *case.box, rtol=1e-8, panels=(5, 3))
    assert _bits(again.value) == _bits(cached.value) == before[0] and again.evals == cached.evals


# ------------------------------------------------------------------ 6. surfaces agree
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def _py(*args):
    return subprocess.run([sys.executable, "-m", "cuda_v_mpi_amd", "integrate", *args], cwd=REPO,
                          capture_output=True, text=True, timeout=300)


SURFACE = rc.PEAK_IN_DISC
FLAGS = ("--expr", SURFACE.expr, "--a", "-1", "--b", "1", f"--y-lo={SURFACE.y_lo}",
         f"--y-hi={SURFACE.y_hi}", "--area-rtol", "1e-8", "--panels", "5", "--panels-y", "3")
JSON_KEYS = ("value", "err_est", "resabs", "tol", "converged", "evals", "rounds", "intervals",
             "splits", "splits_x", "splits_y", "floor", "forced", "nonfinite", "capped",
             "device_ms", "y_lo", "y_hi")


@pytest.fixture(scope="module")
def surface_value():
    """kernels.quad_expr2d_region's result for FLAGS: what every other surface has to print."""
    return _quad(SURFACE, rtol=1e-8, panels=(5, 3))


def _same(js, r):
    for k in JSON_KEYS:
        assert k in js, k
    assert _bits(js["value"]) == _bits(r.value) and js["value_bits"] == _bits(r.value)
    assert js["err_est"] == r.err_est and js["resabs"] == r.resabs and js["tol"] == r.tol
    for k in ("evals", "rounds", "intervals", "splits", "splits_x", "splits_y"):
        assert js[k] == getattr(r, k), k
    assert (js["y_lo"], js["y_hi"]) == (SURFACE.y_lo, SURFACE.y_hi)


def test_native_object_python_api_and_native_cli_agree_bit_for_bit(surface_value):
    r = surface_value
    assert r.converged and abs(r.value - SURFACE.truth) <= rc.value_bound(r)
    m = native()
    obj = m.ExprAdaptiveRegion(*SURFACE.triple, 0).integrate(
        -1.0, 1.0, m.Adapt2DOptions(rtol=1e-8, panels_x=5, panels_y=3))
    api = integrate_expr2d_region(SURFACE.expr, -1.0, 1.0, SURFACE.y_lo, SURFACE.y_hi, rtol=1e-8,
                                  panels_x=5, panels_y=3, backend="hip")
    assert isinstance(api, AdaptiveRegionResult) and api.backend == "hip"
    assert (api.ay, api.by, api.y_lo, api.y_hi) == (0.0, 1.0, SURFACE.y_lo, SURFACE.y_hi)
    for other in (obj, api):
        assert _bits(other.value) == _bits(r.value) and _bits(other.err_est) == _bits(r.err_est)
        assert other.evals == r.evals and other.splits_x == r.splits_x and other.converged
    p = _riemann(*FLAGS, "--json")
    assert p.returncode == 0 and "not converged" not in p.stderr, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    _same(js, r)
    assert (js["ya"], js["yb"]) == (0.0, 1.0)


def test_python_cli_agrees_bit_for_bit(surface_value):
    p = _py(*FLAGS, "--json")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    _same(js, surface_value)
    assert (js["ay"], js["by"]) == (0.0, 1.0)


def test_clis_print_the_value_and_warn_when_not_converged():
    """The plain form prints the value alone; not converged: one warning line on stderr."""
    flags = (*FLAGS[:10], "--panels", "17", "--panels-y", "16", "--max-depth", "0")
    r = _quad(SURFACE, rtol=1e-8, panels=(17, 16), max_depth=0)
    assert not r.converged and r.forced >= 1 and r.rounds == 1
    for p in (_riemann(*flags), _py(*flags)):
        assert p.returncode == 0, p.stderr
        assert len([ln for ln in p.stderr.splitlines() if "not converged" in ln]) == 1, p.stderr
        assert _bits(float(p.stdout.strip().splitlines()[-1])) == _bits(r.value)
