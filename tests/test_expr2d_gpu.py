"""Exact tests of the 2-D run-time expression kernels (csrc/runtime/expr2d.cpp,
ExprIntegrator2D): every value is compared bit for bit with an integer reference, no
tolerance.

The expressions are polynomials in x and y with integer coefficients, |x - y| and the
indicator of a dyadic disc on 2**-k grids (expr2d_cases.py; test_expr2d_cpu.py shows on any
box that each keeps its budget), so both coordinates, every step of the expression, the
column accumulators, the wave and workgroup sums, the partials, their sum and the final
scaling by a power of two are exact in any order: a value must have the bits of the integer
sum. A sample dropped or doubled at a lane, panel, stretch, item or workgroup edge, a column
past nx evaluated, a row index truncated to 32 bits: each moves a value by at least one unit.
One transcendental integrand is held to a derived rounding bound instead.
"""
from __future__ import annotations

import json
import os
import subprocess

import pytest

import expr2d_cases as c2
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def integrator(native, cuda):
    made = {}

    def get(expr: str, grid: int = 0):
        if (expr, grid) not in made:
            made[expr, grid] = native.ExprIntegrator2D(expr, cuda.index, grid)
        return made[expr, grid]
    return get


def _one(native, ei, c, rule, row_begin=None, row_count=None, scale=1.0, comm=None):
    b, m = c.rows
    b, m = (b if row_begin is None else row_begin), (m if row_count is None else row_count)
    return ei.integrate(*c2.launch_args(c), getattr(native.Rule, rule), b, m, scale, comm)


def _same(got, want, what):
    assert c2.bits(got) == c2.bits(want), f"{what}: got {got!r} want {want!r}"


# ------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", c2.SMALL_CASES, ids=lambda c: c.name)
def test_small_cases_every_rule_grid_and_scale(native, integrator, case):
    for grid in c2.GRIDS:
        ei = integrator(case.expr, grid)
        for rule in c2.RULES:
            for scale in c2.SCALES:
                _same(_one(native, ei, case, rule, scale=scale),
                      c2.value(case, rule, scale=scale), f"{case.name} {rule} grid {grid} x{scale}")
    assert c2.value(c2.DISC, "mid") == c2.DISC_MID_COUNT * 2.0 ** -8


# ------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("grid", c2.GRIDS)
def test_lane_layout_edges(native, integrator, grid):
    ei = integrator(c2.SADDLE_EXPR, grid)
    for nx in c2.EDGE_NX:
        c = c2.saddle(nx, c2.EDGE_NY)
        for rows in c2.EDGE_ROWS:
            for rule in ("left", "mid"):
                _same(_one(native, ei, c, rule, c2.EDGE_ROW_BEGIN, rows),
                      c2.value(c, rule, c2.EDGE_ROW_BEGIN, rows), f"{nx} x {rows} {rule}")


@pytest.mark.parametrize("grid", c2.GRIDS)
def test_shape_edges_from_the_shape_function(native, integrator, grid):
    """Launches that sit on, one short of or one past a panel boundary and a lane-turn
    boundary of the shape they themselves run with (expr2d_cases.shape_edges: one for every
    such place expr2d_shape offers at this cap; test_expr2d_cpu.py shows what they cover)."""
    ei = integrator(c2.SADDLE_EXPR, grid)
    for sig, (nx, rows) in c2.shape_edges(native, grid).items():
        c = c2.edge_rule(nx, rows)
        _same(_one(native, ei, c, "mid", c2.EDGE_ROW_BEGIN, rows),
              c2.value(c, "mid", c2.EDGE_ROW_BEGIN, rows), f"{nx} x {rows}: {sig}")


# ------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("case", c2.PLANES, ids=lambda c: c.name)
def test_planes_skinny_and_large(native, integrator, case):
    for grid in (0, 3, 7):
        ei = integrator(case.expr, grid)
        for rule in c2.RULES:
            _same(_one(native, ei, case, rule), c2.value(case, rule), f"{case.name} {rule} {grid}")


# ------------------------------------------------------------------------------ 4
def test_rank_slices_each_exact_and_sum_to_the_whole(native, integrator):
    c = c2.SLICE_CASE
    ei = integrator(c.expr)
    for rule in c2.RULES:
        total = 0
        for b, m in c2.rank_slices(c.ay.n):
            _same(_one(native, ei, c, rule, b, m), c2.value(c, rule, b, m), f"rows {b}+{m}")
            total += c2.exact_total(c, rule, b, m)[0]
        assert total == c2.exact_total(c, rule, 0, c.ay.n)[0]
        _same(_one(native, ei, c, rule), c2.value(c, rule), f"whole {rule}")


# ------------------------------------------------------------------------------ 5, 6
@pytest.mark.parametrize("world", c2.LOOPBACK_WORLDS)
def test_loopback_ranks_get_the_whole_rule(native, cuda, world):
    c = c2.SLICE_CASE
    for rule in c2.RULES:
        def body(rank, comm):
            ei = native.ExprIntegrator2D(c.expr, cuda.index, 0)
            b, m = c2.rank_slices(c.ay.n, world)[rank]
            return _one(native, ei, c, rule, b, m, 1.0, comm)
        out = loopback.run_ranks(world, body)
        want = c2.value(c, rule)
        print(f"{rule}: ranks {out!r} want {want!r}")
        assert out == [want] * world


def test_world_larger_than_ny_idle_rank_adds_zero(native, cuda, integrator):
    c = c2.saddle(1025, 2)
    slices = c2.rank_slices(2, 3)
    assert slices[2][1] == 0
    _same(_one(native, integrator(c.expr), c, "mid", *slices[2]), 0.0, "no rows")

    def body(rank, comm):
        ei = native.ExprIntegrator2D(c.expr, cuda.index, 0)
        return _one(native, ei, c, "mid", *slices[rank], 1.0, comm)
    assert loopback.run_ranks(3, body) == [c2.value(c, "mid")] * 3


# ------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("case", c2.PAST_2_32, ids=lambda c: c.name)
def test_indices_past_2_32(native, integrator, case):
    for grid in (0, 3):
        ei = integrator(case.expr, grid)
        for rule in c2.RULES:
            _same(_one(native, ei, case, rule), c2.value(case, rule), f"{case.name} {rule} {grid}")


# ------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("case", c2.REVERSED, ids=lambda c: c.name)
def test_reversed_intervals(native, integrator, case):
    assert (case.ax.b < case.ax.a) or (case.ay.b < case.ay.a)
    for grid in (0, 3):
        ei = integrator(case.expr, grid)
        for rule in c2.RULES:
            _same(_one(native, ei, case, rule), c2.value(case, rule), f"{case.name} {rule}")
            _same(_one(native, ei, case, rule, 5, 17), c2.value(case, rule, 5, 17), "rows 5+17")
        _same(_one(native, ei, case, "mid", case.ay.n, 0), 0.0, "no rows: +0.0")


# ------------------------------------------------------------------------------ 9, 10
def _depth_2d(native, nx, rows, grid=0):
    """Additions on the longest path from a sample to the value, read off expr2d.cpp: a
    column accumulator takes rows-per-lane samples per item over the workgroup's items,
    (a0 + a1) + (a2 + a3) is 2, the wave butterfly 6, the four wave partials 2; the closing
    kernel's thread adds ceil(workgroups / 256) partials, then 6 and 2 again."""
    s = native.expr2d_shape(nx, rows, grid)
    return s.lane_samples // s.cols_per_lane + 2 + 6 + 2 + -(-s.workgroups // 256) + 6 + 2


def test_coordinates_have_the_1d_bits(native, cuda, integrator):
    """exp(-x*x) has no y: one row of a 2-D rule with hy = 1 sums the samples ExprIntegrator
    sums, at the same coordinates and through the same exp, so the two differ by the order of
    their additions alone: at most (D2 + D1) * 2**-53 * |hx| * sum |f|, D2 as in _depth_2d,
    D1 = 27 for ExprIntegrator's 2048 workgroups with at most one sample per lane (1 + 2 + 6
    + 2, then 8 partials per closing thread + 6 + 2). A coordinate one ulp off moves a
    sample by 2 x^2 ulps, far more at the upper end."""
    import math

    import numpy as np

    expr, a, b, nx = "exp(-x*x)", 0.0, 3.0, 253
    one = native.ExprIntegrator(expr, cuda.index)
    two = integrator(expr)
    for rule in c2.RULES:
        v1 = one.integrate(a, b, nx, getattr(native.Rule, rule), 0, nx)
        v2 = two.integrate(a, b, nx, 0.0, 1.0, 1, getattr(native.Rule, rule), 0, 1)
        h = (b - a) / nx
        mag = math.fsum(np.exp(-(np.arange(nx) * h) ** 2).tolist()) * h * 1.01
        bound = (_depth_2d(native, nx, 1) + 27) * 2.0 ** -53 * mag
        print(f"{rule}: |2-D - 1-D| / bound = {abs(v2 - v1) / bound:.3f}")
        assert abs(v2 - v1) <= bound


def test_gauss_reproducible_and_within_rounding_bound(native, integrator):
    """exp(-(x*x + y*y)) on [0, 3]^2, 253 x 131 samples: two runs are bitwise equal and the
    value is within (c * 2**-52 + D * 2**-53) * |hx hy| * sum |f| of math.fsum of numpy's
    values at coordinates formed in rationals and rounded once.

    c = 56 per sample (expr2d_cases.GAUSS_C): one ulp of the device's exp and one of numpy's,
    and for each of the two the roundings of x*x, y*y and their sum (fewer when contracted),
    each at most 2**-53 of an argument below 18, which exp turns into 18 * 2**-53 of f.
    D = 36 for this rule's shape (expr2d_shape(253, 131): 32 lanes along x, 3 columns a
    lane, one stretch of 131 rows over 8 lanes along y, 3 workgroups), from _depth_2d: 17
    rows down a column accumulator + 2 + 6 + 2 in the workgroup, 1 + 6 + 2 in the closing
    kernel. The multiplication by hx * hy, fsum's own rounding and the reference's
    multiplication are three roundings more, covered by the slack of c."""
    ei = integrator(c2.GAUSS_EXPR)
    ax, bx, nx, ay, by, ny = c2.GAUSS
    D = _depth_2d(native, nx, ny)
    assert D == 36
    for rule in c2.RULES:
        r = getattr(native.Rule, rule)
        got = ei.integrate(ax, bx, nx, ay, by, ny, r, 0, ny)
        assert c2.bits(got) == c2.bits(ei.integrate(ax, bx, nx, ay, by, ny, r, 0, ny))
        ref, mag = c2.gauss_reference(rule)
        bound = (c2.GAUSS_C * 2.0 ** -52 + D * 2.0 ** -53) * mag
        print(f"{rule}: |value - ref| / bound = {abs(got - ref) / bound:.4f}")
        assert abs(got - ref) <= bound


# ------------------------------------------------------------------------------ 11
def test_python_api_backends_agree(cuda):
    """integrate_expr2d with hip, cpu and host: bitwise on the saddle; on the Gaussian each
    within (c * 2**-52 + D * 2**-53) * |hx hy| * sum |f| of the reference of test 10, and any
    two of them within the sum of their two bounds. c = 56 as there (every backend forms
    the coordinates with one fma, rounded once). D, the additions on the longest path from a
    sample to the value, read off each backend's code for 253 x 131 samples:
      hip   36, _depth_2d (expr2d.cpp)
      host  302 with one thread (host_source2d in host_expr.cpp): a row is one block of 253
            columns, acc[0] takes 31 samples in the unrolled loop and the 5 left over = 36,
            the tree of the 8 accumulators 3; the compensated step per row rounds twice on
            the path (c = s - comp, t = total + c), 131 rows = 262; the thread sum 1
      cpu   17 (integrate.py, _tree_sum): a row's 253 columns in a tree of depth 8, the 131
            rows of the one chunk in a tree of depth 8, the chunk onto the total 1."""
    from cuda_v_mpi_amd import integrate_expr2d, native as load

    m = load()
    c = c2.SADDLE
    for rule in c2.RULES:
        vals = [integrate_expr2d(c.expr, c.ax.a, c.ax.b, c.ay.a, c.ay.b, c.ax.n, c.ay.n,
                                 rule=rule, backend=b).value for b in ("hip", "cpu", "host")]
        assert c2.bits(vals) == c2.bits([c2.value(c, rule)] * 3), (rule, vals)
        _same(kernels.riemann_expr2d(c.expr, *c2.launch_args(c), rule=rule), vals[0], "kernels")
        _same(kernels.riemann_expr2d(c.expr, *c2.launch_args(c), rule=rule, row_begin=5, rows=17,
                                     grid=3), c2.value(c, rule, 5, 17), "kernels rows")
    ax, bx, nx, ay, by, ny = c2.GAUSS
    r = integrate_expr2d(c2.GAUSS_EXPR, ax, bx, ay, by, nx, ny, backend="hip", analytic=0.7853)
    assert r.n == nx * ny and r.integrand == "expr2d:" + c2.GAUSS_EXPR and r.gpus == 1
    assert r.rule == "mid" and r.abs_err == abs(r.value - 0.7853)
    ref, mag = c2.gauss_reference("mid")
    assert _depth_2d(m, nx, ny) == 36 and (nx - 1).bit_length() == (ny - 1).bit_length() == 8
    vals, bounds = {}, {}
    for backend, D in (("hip", 36), ("cpu", 8 + 8 + 1), ("host", 36 + 3 + 2 * ny + 1)):
        vals[backend] = integrate_expr2d(c2.GAUSS_EXPR, ax, bx, ay, by, nx, ny, backend=backend,
                                         threads=1).value
        bounds[backend] = (c2.GAUSS_C * 2.0 ** -52 + D * 2.0 ** -53) * mag
        print(f"{backend}: |value - ref| / bound = "
              f"{abs(vals[backend] - ref) / bounds[backend]:.4f}")
        assert abs(vals[backend] - ref) <= bounds[backend], backend
    for p, q in (("hip", "cpu"), ("hip", "host"), ("cpu", "host")):
        assert abs(vals[p] - vals[q]) <= bounds[p] + bounds[q], (p, q)
    sq = integrate_expr2d(c2.GAUSS_EXPR, ax, bx, ay, by, 64)
    assert sq.n == 64 * 64


# ------------------------------------------------------------------------------ 12
def test_refusals_raise_before_any_launch(native, cuda, integrator):
    c = c2.SADDLE
    ei = integrator(c.expr)
    args = c2.launch_args(c)
    mid = native.Rule.mid
    for rows, words in (((30, 8), ("30", "8", "37")), ((38, 0), ("38",)),
                        ((2 ** 64 - 2, 5), (str(2 ** 64 - 2),))):
        with pytest.raises(RuntimeError, match="outside") as e:
            ei.integrate(*args, mid, *rows)
        assert all(w in str(e.value) for w in words)
    with pytest.raises(RuntimeError, match=str(2 ** 32)):
        ei.integrate(0.0, 1.0, 2 ** 32, 0.0, 1.0, 4, mid, 0, 4)
    with pytest.raises(RuntimeError, match=str(2 ** 40 + 1)):
        ei.integrate(0.0, 1.0, 4, 0.0, 1.0, 2 ** 40 + 1, mid, 0, 4)
    with pytest.raises(RuntimeError, match="32-bit") as e:
        integrator(c.expr, 1).integrate(0.0, 1.0, 2 ** 20, 0.0, 1.0, 2 ** 40, mid, 0, 2 ** 40)
    assert "1048576" in str(e.value) and str(2 ** 40) in str(e.value)
    with pytest.raises(RuntimeError, match="32-bit"):
        integrator(c.expr, 1).time(0.0, 1.0, 2 ** 20, 0.0, 1.0, 2 ** 40, mid, 0, 2 ** 40, 1)
    with pytest.raises(RuntimeError, match="grid"):
        native.ExprIntegrator2D(c.expr, cuda.index, 2049)
    # the object still integrates after the refusals
    _same(_one(native, ei, c, "mid"), c2.value(c, "mid"), "after refusals")
    assert ei.time(*args, mid, 0, c.ay.n, 2) > 0


def test_objects_own_their_loaded_module(native, cuda):
    """The smallest case at grid 3: A and B for one expression, A destroyed, a fresh C."""
    c = min(c2.SMALL_CASES, key=lambda k: k.ax.n * k.ay.n)
    c2.check_module_lifetime(
        lambda: native.ExprIntegrator2D(c.expr, cuda.index, 3),
        lambda ei, what: _same(_one(native, ei, c, "mid"), c2.value(c, "mid"), what))


# ------------------------------------------------------------------------------ 13
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def test_cli_on_the_device(cuda):
    c = c2.SADDLE_TALL
    base = ("--expr", c.expr, "--a", repr(c.ax.a), "--b", repr(c.ax.b), "--ya", repr(c.ay.a),
            "--yb", repr(c.ay.b), "--n", str(c.ax.n), "--ny", str(c.ay.n), "--rule", "mid",
            "--json", "--iters", "2")
    want = c2.value(c, "mid")
    p = _riemann(*base, "--analytic", "2.5")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    _same(js["value"], want, "cli value")
    assert js["expr"] == c.expr and js["a"] == c.ax.a and js["b"] == c.ax.b
    assert js["ya"] == c.ay.a and js["yb"] == c.ay.b and js["n"] == c.ax.n and js["ny"] == c.ay.n
    assert js["rule"] == "mid" and js["gpus"] == 1 and js["comm"] == "none"
    assert js["device_ms"] > 0 and js["samples_per_s"] > 0 and js["abs_err"] == abs(want - 2.5)
    p = _riemann(*base, "--loopback", "3")
    assert p.returncode == 0, p.stderr
    j3 = json.loads(p.stdout.strip().splitlines()[-1])
    _same(j3["value"], want, "cli --loopback 3")
    assert j3["gpus"] == 3 and j3["comm"] == "loopback"
