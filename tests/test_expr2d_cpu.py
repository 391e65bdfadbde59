"""CPU side of the 2-D run-time expression tests: the references against brute force, the
budgets of every case of expr2d_cases.py, the conditions on the launch shape (expr2d_shape
needs no device), the gfx950 compile of the expressions, the host twin (HostExpr2D) bit for
bit on every exact case, the CLI's refusals and the torch form with y."""
from __future__ import annotations

import json
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import expr2d_cases as c2
from cuda_v_mpi_amd.utils import exact_riemann2d as x2
from cuda_v_mpi_amd.utils.exact_riemann2d import Axis

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ references
def _coords(a: Axis, off2: int, begin: int, count: int) -> list:
    h = Fraction(-1 if a.reverse else 1, 2 ** a.k)
    return [Fraction(a.a_num, 2 ** (a.k + 1)) + (i + Fraction(off2, 2)) * h
            for i in range(begin, begin + count)]


def _brute(f, ax: Axis, ay: Axis, off2: int, rb: int, rc: int) -> Fraction:
    xs, ys = _coords(ax, off2, 0, ax.n), _coords(ay, off2, rb, rc)
    return sum((f(x, y) for y in ys for x in xs), Fraction(0))


@pytest.mark.parametrize("reverse", [False, True])
def test_references_against_fraction_brute_force(reverse):
    ax, ay = Axis(3, c2.a_num_R(3, 2), 13), Axis(3, c2.a_num_of(3), 11)
    if reverse:
        ax, ay = c2.reversed_axis(ax), c2.reversed_axis(ay)
    assert ax.a == float(_coords(ax, 0, 0, 1)[0]) and ax.b == float(_coords(ax, 0, ax.n, 1)[0])
    for off2 in (0, 1, 2):
        for rb, rc in ((0, 11), (3, 5), (10, 1)):
            tot = x2.exact_poly2d_sum(c2.SADDLE_COEF, ax, ay, off2, rb, rc)
            want = _brute(lambda x, y: 3 * x * y * y - 2 * y * y + 5 * x * y - 7 * x * x + 4,
                          ax, ay, off2, rb, rc)
            assert Fraction(tot, 2 ** x2.poly2d_unit_bits(c2.SADDLE_COEF, ax, ay)) == want
            tot = x2.exact_poly2d_sum(c2.PLANE_COEF, ax, ay, off2, rb, rc)
            want = _brute(lambda x, y: 7 * x - 5 * y + 3, ax, ay, off2, rb, rc)
            assert Fraction(tot, 2 ** x2.poly2d_unit_bits(c2.PLANE_COEF, ax, ay)) == want
            tot = x2.exact_absdiff_sum(3, -2, ax, ay, off2, rb, rc)
            assert Fraction(tot, 2 ** 4) == _brute(lambda x, y: 3 * abs(x - y) - 2, ax, ay,
                                                   off2, rb, rc)
            cnt = x2.exact_disc_count(6400 >> 2, ax, ay, off2, rb, rc)   # k = 3: 6.25 * 2**8
            assert cnt == _brute(lambda x, y: Fraction(int(x * x + y * y < Fraction(25, 4))),
                                 ax, ay, off2, rb, rc)


def test_moment_reference_equals_numpy_broadcast():
    c = c2.SADDLE
    for rule in c2.RULES:
        off2 = c2.OFF2[rule]
        xn = (c.ax.a_num + off2 + 2 * np.arange(c.ax.n, dtype=np.int64))[None, :]
        yn = (c.ay.a_num + off2 + 2 * np.arange(c.ay.n, dtype=np.int64))[:, None]
        sx, sy = c.ax.k + 1, c.ay.k + 1          # unit: 2**-(2 sx + 2 sy)
        grid = (3 * xn * yn * yn << sx) - (2 * yn * yn << 2 * sx) + (5 * xn * yn << sx + sy) \
            - (7 * xn * xn << 2 * sy) + (4 << 2 * sx + 2 * sy)
        assert int(grid.sum()) == x2.exact_poly2d_sum(c.coef, c.ax, c.ay, off2, 0, c.ay.n)


def test_every_case_keeps_its_budget():
    assert {c.name for c in c2.EXACT_CASES} == set(c2.BUDGETS)
    for c in c2.EXACT_CASES + c2.REVERSED:
        b = c2.budget(c)
        print(f"{c.name}: {b:.2f} bits")
        assert b < 53, c.name
        if c.name in c2.BUDGETS:
            assert round(b, 1) == c2.BUDGETS[c.name], c.name
    # the edge rules are the saddle's coordinates with fewer samples: inside its budget
    assert c2.budget(c2.saddle(max(c2.EDGE_NX), c2.EDGE_NY)) <= c2.budget(c2.SADDLE)
    assert x2.exact_disc_count(c2.DISC_R2_NUM, c2.DISC.ax, c2.DISC.ay, 1, 0, 150) \
        == c2.DISC_MID_COUNT
    # every reference value is an fp64 (value_f64 refuses a sum past 2**53)
    for c in c2.EXACT_CASES + c2.REVERSED:
        for rule in c2.RULES:
            assert np.isfinite(c2.value(c, rule))


def test_slices_and_past_2_32_are_what_they_claim():
    assert c2.PAST_FLAT.row_begin * c2.PAST_FLAT.ax.n > 2 ** 32
    assert c2.PAST_ROW.row_begin > 2 ** 32 and c2.PAST_ROW.ay.n == 2 ** 40
    sl = c2.rank_slices(c2.SLICE_CASE.ay.n)
    assert [m for _, m in sl] == [37, 37, 37, 37, 37, 36, 36] and sum(m for _, m in sl) == 257
    assert any(b % 2 for b, _ in sl)
    for rule in c2.RULES:   # the slices' integer sums add up to the whole
        parts = [c2.exact_total(c2.SLICE_CASE, rule, b, m)[0] for b, m in sl]
        assert sum(parts) == c2.exact_total(c2.SLICE_CASE, rule, 0, 257)[0]


# ------------------------------------------------------------------------------ launch shape
def _fill(native, nx, rows, grid=0):
    s = native.expr2d_shape(nx, rows, grid)
    lx, cpl = s.lanes_x, s.cols_per_lane
    ly = c2.BLOCK // lx
    # the struct is consistent with the kernel's dealing
    assert lx in (1, 2, 4, 8, 16, 32, 64, 128, 256) and 1 <= cpl <= 4
    assert s.panels == -(-nx // (lx * cpl)) and s.items == s.panels * s.stretches
    assert s.rows_per_item == -(-rows // s.stretches)
    assert s.items_per_wg == -(-s.items // (grid or native.EXPR2D_MAX_GRID))
    assert s.workgroups == -(-s.items // s.items_per_wg) <= (grid or native.EXPR2D_MAX_GRID)
    assert s.lane_samples == cpl * -(-s.rows_per_item // ly) * s.items_per_wg < 2 ** 32
    assert s.as_tuple() == (lx, cpl, s.rows_per_item, s.items, s.items_per_wg, s.workgroups)
    return nx * rows / (s.workgroups * c2.BLOCK * s.lane_samples)


def test_shape_fills_more_than_half_of_its_slots(native):
    """Condition 2: for nx * row_count >= 2**20 more than half of workgroups * 256 * the
    largest per-lane sample count are real samples. nx from 1 to 5000 with the least
    row_count that reaches 2**20, both skinny rules, and random shapes."""
    worst = 1.0
    for nx in range(1, 5001):
        worst = min(worst, _fill(native, nx, -(-(1 << 20) // nx)))
    for rows in list(range(1, 300)) + [1000, 4097]:
        worst = min(worst, _fill(native, -(-(1 << 20) // rows), rows))
    for nx, rows in ((3, 10 ** 7), (10 ** 7, 3), (32768, 32768), (1, 2 ** 40), (2 ** 32 - 1, 1),
                     (2 ** 20, 2 ** 20)):
        worst = min(worst, _fill(native, nx, rows))
    rnd = random.Random(16)
    for _ in range(3000):
        nx = int(2 ** rnd.uniform(0, 31.9))
        rows = max(-(-(1 << 20) // nx), int(2 ** rnd.uniform(0, 44 - np.log2(nx))))
        worst = min(worst, _fill(native, nx, min(rows, 2 ** 40)))
    for grid in (1, 3, 7, 256):
        for nx, rows in ((4099, 2053), (3, 400003), (400003, 3), (1025, 1025), (300, 7001)):
            worst = min(worst, _fill(native, nx, rows, grid))
    print(f"smallest fill {worst:.3f}")
    assert worst > 0.5


def test_shape_is_a_function_of_nx_rows_grid_only(native):
    """Condition 1: expr2d_shape takes (nx, row_count, grid) and nothing else, and the shape
    ExprIntegrator2D launches a slice with (expr2d_plan: the one call integrate and time make,
    with row_begin among its arguments) is that shape wherever the slice begins."""
    with pytest.raises(TypeError):
        native.expr2d_shape(1025, 37, 0, 5)
    fields = ("lanes_x", "cols_per_lane", "rows_per_item", "stretches", "panels", "items",
              "items_per_wg", "workgroups", "lane_samples")

    def whole(s):
        return tuple(getattr(s, f) for f in fields)
    for nx, ny, rows, grid in ((1025, 37, 17, 0), (300, 257, 36, 3), (4099, 2053, 293, 0),
                               (4099, 2053, 293, 7), (1025, 2 ** 40, 5, 0), (3, 40003, 5000, 1)):
        want = whole(native.expr2d_shape(nx, rows, grid))
        for begin in (0, 1, 5, (ny - rows) // 2, ny - rows - 1, ny - rows):
            assert whole(native.expr2d_plan(nx, ny, begin, rows, grid)) == want, (nx, ny, begin)
    idle = native.expr2d_plan(1025, 37, 37, 0, 0)
    assert idle.workgroups == 0 and idle.items == 0 and idle.lane_samples == 0
    with pytest.raises(RuntimeError, match="outside"):
        native.expr2d_plan(1025, 37, 30, 8, 0)


def test_shapes_the_gpu_tests_assume(native):
    """What test_expr2d_gpu.py leans on: the skinny rules fold the lanes onto the long axis,
    the large plane at a cap of 3 and 7 gives workgroups several items with a ragged last
    one, the small cases cover every column count 1..4 and a partly filled panel, and an
    over-full per-lane count at one workgroup is refused with the numbers named."""
    sx = native.expr2d_shape(3, 40003, 0)
    sy = native.expr2d_shape(40003, 3, 0)
    assert sx.lanes_x == 1 and sx.cols_per_lane == 3 and sx.workgroups > 1
    assert sy.lanes_x == 256 and sy.rows_per_item == 3 and sy.workgroups > 1
    for grid in (3, 7):
        s = native.expr2d_shape(4099, 2053, grid)
        assert s.items_per_wg > 1 and s.workgroups == grid
        assert 4099 % (s.lanes_x * s.cols_per_lane), "the last panel is partly filled"
        assert s.cols_per_lane == 4
    s = native.expr2d_shape(4099, 2053, 7)
    assert s.items % s.items_per_wg and s.stretches > 1, "a ragged last run, several stretches"
    assert native.expr2d_shape(2 ** 20, 3, 3).items_per_wg > 1
    # the shape-edge launches: each on an edge of the shape it itself runs with, inside the
    # budget, and between them every column count, both sides of a panel and of a lane turn,
    # more than one panel and (at a cap of one workgroup) more than one item per workgroup
    assert c2.budget(c2.edge_rule(c2.SHAPE_EDGE_NX, c2.SHAPE_EDGE_ROWS)) < 53
    for grid in c2.GRIDS:
        edges = c2.shape_edges(native, grid)
        for sig, (nx, rows) in edges.items():
            assert c2.own_edge(native, nx, rows, grid) == sig
            s = native.expr2d_shape(nx, rows, grid)
            panel, ly = s.lanes_x * s.cols_per_lane, c2.BLOCK // s.lanes_x
            assert min(nx % panel, panel - nx % panel) <= 1
            assert min(s.rows_per_item % ly, ly - s.rows_per_item % ly) <= 1
        sigs = set(edges)
        print(f"grid {grid}: {len(sigs)} shape-edge launches")
        assert {g[1] for g in sigs} == {1, 2, 3, 4}
        assert {g[2] for g in sigs} == {-1, 0, 1} and {g[3] for g in sigs} == {-1, 0, 1}
        assert {g[4] for g in sigs} == {1, 2}
        assert len({g[0] for g in sigs}) >= 5
    assert any(native.expr2d_shape(nx, rows, 1).items_per_wg > 1
               for nx, rows in c2.shape_edges(native, 1).values())
    cols = set()
    for grid in c2.GRIDS:
        for nx in c2.EDGE_NX:
            for rows in c2.EDGE_ROWS:
                cols.add(native.expr2d_shape(nx, rows, grid).cols_per_lane)
    assert cols == {1, 2, 3, 4}
    with pytest.raises(RuntimeError, match="32-bit") as e:
        native.expr2d_check(2 ** 20, 2 ** 40, 0, 2 ** 40, 1)
    assert "1048576" in str(e.value) and "1099511627776" in str(e.value)


def test_check_refuses_what_the_kernels_cannot_index(native):
    native.expr2d_check(1025, 37, 5, 17, 0)
    native.expr2d_check(1025, 37, 37, 0, 0)           # an idle rank: no rows, at the end
    native.expr2d_check(2 ** 32 - 1, 2 ** 40, 2 ** 40 - 1, 1, 0)
    for args, words in (((1025, 37, 30, 8, 0), ("30", "8", "37")),
                        ((1025, 37, 38, 0, 0), ("38", "37")),
                        ((1025, 37, 2 ** 64 - 2, 5, 0), (str(2 ** 64 - 2), "37")),
                        ((2 ** 32, 37, 0, 37, 0), (str(2 ** 32),)),
                        ((0, 37, 0, 37, 0), ("nx = 0",)),
                        ((1025, 2 ** 40 + 1, 0, 5, 0), (str(2 ** 40 + 1),)),
                        ((1025, 0, 0, 0, 0), ("ny = 0",))):
        with pytest.raises(RuntimeError) as e:
            native.expr2d_check(*args)
        assert all(w in str(e.value) for w in words), (args, str(e.value))


# ------------------------------------------------------------------------------ compile
@pytest.mark.parametrize("expr", c2.EXPRESSIONS + (c2.GAUSS_EXPR, "exp(-x*x)"))
def test_compile_for_gfx950_without_a_device(native, expr):
    code = native.expr2d_compile(expr)
    assert code[:4] == b"\x7fELF" and b"miint_expr2d_partials" in code \
        and b"miint_expr2d_finalize" in code
    assert expr in native.expr2d_source(expr)


@pytest.mark.parametrize("expr", ["x; y", "asm(x)", "x+z"])
def test_rejected_expressions_name_the_expression(native, expr):
    with pytest.raises(RuntimeError) as e:
        native.expr2d_compile(expr)
    msg = str(e.value)
    assert f"'{expr}'" in msg, msg
    assert ("not allowed" in msg) if expr != "x+z" else ("z" in msg.replace(expr, ""))
    with pytest.raises(RuntimeError) as e:
        native.expr2d_source(expr) if expr != "x+z" else native.HostExpr2D(expr)
    assert f"'{expr}'" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        native.HostExpr2D(expr)
    assert f"'{expr}'" in str(e.value) and (expr == "x+z" or "not allowed" in str(e.value))


# ------------------------------------------------------------------------------ host twin
@pytest.fixture(scope="module")
def pools(native):
    return {t: native.HostPool(t) for t in (1, 3, 4)}


@pytest.mark.parametrize("case", c2.EXACT_CASES + c2.REVERSED, ids=lambda c: c.name)
def test_host_twin_is_exact(native, pools, case):
    he = native.HostExpr2D(case.expr)
    b, m = case.rows
    for rule in c2.RULES:
        want = c2.value(case, rule)
        for t, pool in pools.items():
            got = he.integrate(*c2.launch_args(case), getattr(native.Rule, rule), b, m, pool)
            assert c2.bits(got) == c2.bits(want), (case.name, rule, t, got, want)
    got = he.integrate(*c2.launch_args(case), native.Rule.mid, b, m, pools[3], 2.0 ** -3)
    assert c2.bits(got) == c2.bits(c2.value(case, "mid", scale=2.0 ** -3))


def test_host_twin_slices_edges_and_refusals(native, pools):
    c = c2.SLICE_CASE
    he = native.HostExpr2D(c.expr)
    for rule in c2.RULES:
        for b, m in c2.rank_slices(c.ay.n):
            got = he.integrate(*c2.launch_args(c), getattr(native.Rule, rule), b, m, pools[3])
            assert c2.bits(got) == c2.bits(c2.value(c, rule, b, m))
    assert he.integrate(*c2.launch_args(c), native.Rule.mid, 257, 0, pools[3]) == 0.0
    for r in c2.REVERSED:   # no rows: +0.0 whatever the signs of the steps
        zero = native.HostExpr2D(r.expr).integrate(*c2.launch_args(r), native.Rule.mid, 37, 0,
                                                   pools[3])
        assert c2.bits(zero) == c2.bits(0.0), r.name
    for nx in c2.EDGE_NX:
        e = c2.saddle(nx, c2.EDGE_NY)
        for rows in c2.EDGE_ROWS:
            got = he.integrate(*c2.launch_args(e), native.Rule.mid, c2.EDGE_ROW_BEGIN, rows,
                               pools[4])
            assert c2.bits(got) == c2.bits(c2.value(e, "mid", c2.EDGE_ROW_BEGIN, rows))
    for args in ((250, 8), (2 ** 64 - 2, 5)):
        with pytest.raises(RuntimeError, match="outside"):
            he.integrate(*c2.launch_args(c), native.Rule.mid, *args, pools[1])
    # an expression without y compiles: the rows repeat the 1-D sum
    one = native.HostExpr("exp(-x*x)").integrate(0.0, 3.0, 253, native.Rule.mid, 0, 253, pools[1])
    two = native.HostExpr2D("exp(-x*x)").integrate(0.0, 3.0, 253, 0.0, 1.0, 1, native.Rule.mid,
                                                   0, 1, pools[1])
    assert abs(two - one) <= 4 * 2.0 ** -52 * abs(one)


# ------------------------------------------------------------------------------ python
def test_expr_torch_with_y_and_unchanged_without():
    from cuda_v_mpi_amd import integrate_expr2d
    from cuda_v_mpi_amd.integrate import expr_torch

    x = torch.linspace(-1.0, 2.0, 7, dtype=torch.float64)
    y = torch.linspace(0.5, 1.5, 3, dtype=torch.float64).unsqueeze(1)
    got = expr_torch("exp(-(x*x+y*y))*cos(x*y)+2.0", x, y)
    assert got.shape == (3, 7)
    assert torch.equal(got, torch.exp(-(x * x + y * y)) * torch.cos(x * y) + 2.0)
    assert expr_torch("3.0", x, y).shape == (3, 7)
    assert expr_torch("x*x", x, y).shape == (3, 7)
    # 1-D calls are what they were: same values, y an unknown name
    assert torch.equal(expr_torch("exp(-x*x)+1.0", x), torch.exp(-x * x) + 1.0)
    with pytest.raises(ValueError, match="does not evaluate"):
        expr_torch("x*y", x)
    # the torch backend of integrate_expr2d on the saddle: the exact value, on any box
    c = c2.SADDLE
    for rule in c2.RULES:
        r = integrate_expr2d(c.expr, c.ax.a, c.ax.b, c.ay.a, c.ay.b, c.ax.n, c.ay.n, rule=rule,
                             backend="cpu")
        assert c2.bits(r.value) == c2.bits(c2.value(c, rule))
        assert r.n == c.ax.n * c.ay.n and r.integrand == "expr2d:" + c.expr and r.gpus == 1
    r = integrate_expr2d(c.expr, c.ax.a, c.ax.b, c.ay.a, c.ay.b, c.ax.n, c.ay.n, rule="mid",
                         backend="host", threads=3)
    assert c2.bits(r.value) == c2.bits(c2.value(c, "mid"))
    with pytest.raises(ValueError, match="backend"):
        integrate_expr2d(c.expr, 0, 1, 0, 1, 4, backend="numpy")


def test_fma_coords_have_the_fma_bits():
    """The torch backend's coordinates (formed on the host with one fma each) against fma in
    rationals, on steps that are not dyadic and far row indices."""
    from cuda_v_mpi_amd.integrate import _fma_coords

    for a, h, first, off in ((0.0, 3.0 / 253, 0, 0.5), (-2.7, 3.3 / 131, 5, 1.0),
                             (1e-3, 1.0 / 3.0, 2 ** 33 + 1, 0.5), (0.1, -0.7 / 97, 11, 0.0)):
        got = _fma_coords(first, 200, off, h, a).tolist()
        want = [float(Fraction(a) + (Fraction(i) + Fraction(off)) * Fraction(h))
                for i in range(first, first + 200)]
        assert got == want


# ------------------------------------------------------------------------------ CLI
def _riemann(*args):
    exe = os.path.join(REPO, "build", "bin", "riemann")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", REPO, "-j8", "cli"], check=True, capture_output=True)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)


def _saddle_args(c=c2.SADDLE):
    return ("--expr", c.expr, "--a", repr(c.ax.a), "--b", repr(c.ax.b), "--ya", repr(c.ay.a),
            "--yb", repr(c.ay.b), "--n", str(c.ax.n), "--ny", str(c.ay.n))


def test_cli_refusals_and_help():
    base = _saddle_args()
    for extra, words in ((("--running",), ("--running", "--ya")),
                         (("--params", "rows.txt"), ("--params", "--linspace")),
                         (("--linspace", "p0=0:1:3"), ("--params", "--linspace"))):
        p = _riemann(*base, "--device", "cpu", *extra)
        assert p.returncode == 1 and all(w in p.stderr for w in words), (extra, p.stderr)
    p = _riemann("--expr", "x*y", "--a", "0", "--b", "1", "--ya", "0", "--device", "cpu")
    assert p.returncode == 1 and "--ya" in p.stderr and "--yb" in p.stderr
    p = _riemann("--expr", "x*y", "--a", "0", "--b", "1", "--yb", "2", "--device", "cpu")
    assert p.returncode == 1 and "--ya" in p.stderr and "--yb" in p.stderr
    p = _riemann("--expr", "x*x", "--a", "0", "--b", "1", "--ny", "5", "--device", "cpu")
    assert p.returncode == 1 and "--ny" in p.stderr
    p = _riemann("--ya", "0", "--yb", "1", "--device", "cpu")
    assert p.returncode == 1 and "--expr" in p.stderr
    p = _riemann("--help")
    assert p.returncode == 0
    for w in ("--ya AY", "--yb BY", "--ny NY", "double integral"):
        assert w in p.stdout, w


def test_cli_device_cpu_prints_the_saddles_value():
    c = c2.SADDLE
    p = _riemann(*_saddle_args(), "--rule", "mid", "--device", "cpu", "--threads", "3", "--json",
                 "--analytic", "1.5")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    want = c2.value(c, "mid")
    assert c2.bits(js["value"]) == c2.bits(want)
    assert js["expr"] == c.expr and js["a"] == c.ax.a and js["b"] == c.ax.b
    assert js["ya"] == c.ay.a and js["yb"] == c.ay.b and js["n"] == c.ax.n and js["ny"] == c.ay.n
    assert js["rule"] == "mid" and js["device"] == "cpu" and js["threads_per_rank"] == 3
    assert js["abs_err"] == abs(want - 1.5) and js["host_ms"] > 0 and js["samples_per_s"] > 0
    # --ny defaults to --n, and the two-line form names both intervals
    sq = c2.saddle(37, 37)
    p = _riemann("--expr", sq.expr, "--a", repr(sq.ax.a), "--b", repr(sq.ax.b), "--ya",
                 repr(sq.ay.a), "--yb", repr(sq.ay.b), "--n", "37", "--device", "cpu", "--json")
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert js["ny"] == 37 and c2.bits(js["value"]) == c2.bits(c2.value(sq, "left"))
    assert "f(x, y)" in p.stdout and "37 x 37" in p.stdout


def test_python_cli_integrate_takes_the_2d_flags():
    c = c2.saddle(65, 17)
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, "-m", "cuda_v_mpi_amd", "integrate", "--expr", c.expr,
           f"--a={c.ax.a!r}", f"--b={c.ax.b!r}", f"--ya={c.ay.a!r}", f"--yb={c.ay.b!r}",
           "--n", "65", "--ny", "17", "--rule", "mid", "--device", "cpu"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr
    js = json.loads(p.stdout.strip().splitlines()[-1])
    assert c2.bits(js["value"]) == c2.bits(c2.value(c, "mid"))
    assert js["n"] == 65 and js["ny"] == 17 and js["ya"] == c.ay.a and js["yb"] == c.ay.b
    lone = [sys.executable, "-m", "cuda_v_mpi_amd", "integrate", "--expr", "x*y", "--a=0", "--b=1",
            "--ya=0", "--device", "cpu"]
    p = subprocess.run(lone, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert p.returncode != 0 and "--yb" in p.stderr
