"""The inputs of the exact tests of the 2-D run-time expression kernels, in one place:
test_expr2d_gpu.py launches them on the device (ExprIntegrator2D, kernels.riemann_expr2d,
integrate_expr2d, the riemann CLI), test_expr2d_cpu.py asserts on any box that every one of
them keeps its exactness budget (exact_riemann2d) and the structural facts the GPU tests lean
on, and runs the host twin (HostExpr2D) on them.

Coordinates per axis as in expr_exact_cases.py: a step 2**-k from a = a_num / 2**(k+1) with
a = -2.625 - 5 h (a_num_of) or -R - 1/8 - 5 h (a_num_R), so that no lane run starts on a
round number. Every expression is a polynomial in x and y with integer coefficients, an
absolute value of a difference of coordinates or an indicator of a dyadic disc: nothing any
kernel forms from them can round, so every value must have the bits of the integer sum.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from cuda_v_mpi_amd.parallel.decomposition import rank_slice
from cuda_v_mpi_amd.utils import exact_riemann2d as x2
from cuda_v_mpi_amd.utils.exact_riemann2d import Axis

from expr_exact_cases import (LOOPBACK_WORLDS, OFF2, RULES, WORLD, a_num_R,  # noqa: F401
                              a_num_of, bits, check_module_lifetime)

BLOCK = 256                    # threads of a workgroup of the 2-D kernels
GRIDS = (1, 3, 0)              # workgroup caps: one, three, 0 = the auto shape (2048)
SCALES = (1.0, 2.0 ** -3)


class Case(NamedTuple):
    name: str
    expr: str            # what the kernels compile
    kind: str            # "poly" (coef: {(p, q): c}), "absdiff" (coef: (p1, p2)), "disc" (r2_num)
    coef: object
    ax: Axis
    ay: Axis
    row_begin: int = 0            # the slice that is launched and that bounds the budget
    row_count: int | None = None  # (the whole rule unless given)

    @property
    def rows(self) -> tuple[int, int]:
        return self.row_begin, self.ay.n - self.row_begin if self.row_count is None else self.row_count


SADDLE_EXPR = "((3.0*x-2.0)*y+5.0*x)*y-7.0*x*x+4.0"      # 3xy^2 - 2y^2 + 5xy - 7x^2 + 4
SADDLE_COEF = {(1, 2): 3, (0, 2): -2, (1, 1): 5, (2, 0): -7, (0, 0): 4}
PLANE_EXPR = "7.0*x-5.0*y+3.0"
PLANE_COEF = {(1, 0): 7, (0, 1): -5, (0, 0): 3}
PLANE0_EXPR = "7.0*x-5.0*y"
PLANE0_COEF = {(1, 0): 7, (0, 1): -5}
DIAGONAL_EXPR = "3.0*fabs(x-y)-2.0"
DISC_EXPR = "(x*x+y*y<6.25)?1.0:0.0"
DISC_R2_NUM = 6400             # 6.25 in units of 2**-(2 (k+1)), k = 4
GAUSS_EXPR = "exp(-(x*x+y*y))"
EXPRESSIONS = (SADDLE_EXPR, PLANE_EXPR, DIAGONAL_EXPR, DISC_EXPR)

SADDLE_X, SADDLE_Y = (5, a_num_R(5, 8)), (4, a_num_R(4, 4))   # (k, a_num) per axis


def saddle(nx: int, ny: int, name: str = "saddle") -> Case:
    return Case(name, SADDLE_EXPR, "poly", SADDLE_COEF, Axis(*SADDLE_X, nx), Axis(*SADDLE_Y, ny))


def plane(nx: int, ny: int, name: str) -> Case:
    return Case(name, PLANE_EXPR, "poly", PLANE_COEF, Axis(2, a_num_of(2), nx),
                Axis(2, a_num_of(2), ny))


SADDLE = saddle(1025, 37, "saddle-1025x37")
SADDLE_TALL = saddle(300, 257, "saddle-300x257")
PLANE_BIG = plane(4099, 2053, "plane-4099x2053")
PLANE_SKINNY_X = plane(3, 40003, "plane-3x40003")
PLANE_SKINNY_Y = plane(40003, 3, "plane-40003x3")
# the kink on the diagonal crosses the grid: x in [-4.44, 4.94), y in [-2.94, 5.25)
DIAGONAL = Case("diagonal", DIAGONAL_EXPR, "absdiff", (3, -2), Axis(4, a_num_R(4, 4), 150),
                Axis(4, a_num_of(4), 131))
DISC = Case("disc", DISC_EXPR, "disc", DISC_R2_NUM, Axis(4, a_num_R(4, 4), 150),
            Axis(4, a_num_R(4, 4), 150))
DISC_MID_COUNT = 5024          # lattice points of the mid rule inside the disc, of 150 x 150
# rows 4097 .. 4099 of the 2^20 x 2^20 rule of step 1: flattened sample indices past 2^32
PAST_FLAT = Case("flat-past-2^32", PLANE0_EXPR, "poly", PLANE0_COEF, Axis(0, 0, 2 ** 20),
                 Axis(0, 0, 2 ** 20), 4097, 3)
# rows 2^33 + 1 .. 2^33 + 5 of the 1025 x 2^40 rule of step 1: row indices past 2^32
PAST_ROW = Case("row-past-2^32", PLANE0_EXPR, "poly", PLANE0_COEF, Axis(0, 0, 1025),
                Axis(0, 0, 2 ** 40), 2 ** 33 + 1, 5)

SMALL_CASES = (SADDLE, DIAGONAL, DISC)                       # every rule, grid and scale
PLANES = (PLANE_SKINNY_X, PLANE_SKINNY_Y, PLANE_BIG)
PAST_2_32 = (PAST_FLAT, PAST_ROW)
EXACT_CASES = (SADDLE, SADDLE_TALL, DIAGONAL, DISC) + PLANES + PAST_2_32

# the budgets of the cases as first computed (bits, one decimal): the CPU test asserts the
# bound itself (< 53) and that none of these moved
BUDGETS = {"saddle-1025x37": 49.7, "saddle-300x257": 50.4, "plane-4099x2053": 42.2,
           "plane-3x40003": 38.5, "plane-40003x3": 39.0, "flat-past-2^32": 46.4,
           "row-past-2^32": 49.6, "diagonal": 24.3, "disc": 15.6}


def budget(c: Case) -> float:
    if c.kind == "poly":
        return x2.expr2d_budget_bits(c.coef, c.ax, c.ay, *c.rows)
    if c.kind == "absdiff":
        return x2.absdiff_budget_bits(*c.coef, c.ax, c.ay)
    return x2.disc_budget_bits(c.ax, c.ay)


def exact_total(c: Case, rule: str, row_begin: int, row_count: int) -> tuple[int, int]:
    """(the integer sum over all columns of the rows, its unit's bits)."""
    if c.kind == "poly":
        return (x2.exact_poly2d_sum(c.coef, c.ax, c.ay, OFF2[rule], row_begin, row_count),
                x2.poly2d_unit_bits(c.coef, c.ax, c.ay))
    if c.kind == "absdiff":
        return (x2.exact_absdiff_sum(*c.coef, c.ax, c.ay, OFF2[rule], row_begin, row_count),
                c.ax.k + 1)
    return x2.exact_disc_count(c.coef, c.ax, c.ay, OFF2[rule], row_begin, row_count), 0


def value(c: Case, rule: str, row_begin: int | None = None, row_count: int | None = None,
          scale: float = 1.0) -> float:
    """S * ((hx * hy) * scale) over all columns of rows [row_begin, row_begin + row_count),
    exactly: the fp64 every launch of the case must return (scale a power of two)."""
    b, n = c.rows
    b, n = (b if row_begin is None else row_begin), (n if row_count is None else row_count)
    if n == 0:
        return 0.0
    tot, unit = exact_total(c, rule, b, n)
    return x2.value_f64(tot, unit) * ((c.ax.h * c.ay.h) * scale)


def launch_args(c: Case) -> tuple:
    """(ax, bx, nx, ay, by, ny) as the integrators take them."""
    return c.ax.a, c.ax.b, c.ax.n, c.ay.a, c.ay.b, c.ay.n


def reversed_axis(a: Axis) -> Axis:
    """The same sample set walked from the other end: a' = b, b' = a, a negative step."""
    return Axis(a.k, a.a_num + 2 * a.n, a.n, True)


REVERSED = (saddle(1025, 37)._replace(name="saddle-reversed-x", ax=reversed_axis(SADDLE.ax)),
            saddle(1025, 37)._replace(name="saddle-reversed-y", ay=reversed_axis(SADDLE.ay)),
            saddle(1025, 37)._replace(name="saddle-reversed-xy", ax=reversed_axis(SADDLE.ax),
                                      ay=reversed_axis(SADDLE.ay)))

# lane-layout edges, on the saddle's coordinates, rows from an odd first row
EDGE_ROW_BEGIN = 5
EDGE_NX = (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
EDGE_ROWS = (1, 2, 5, 17)
EDGE_NY = 37                   # the rule the edge rows are taken from: 5 + 17 <= 37


def edge_rule(nx: int, rows: int) -> Case:
    """The saddle's coordinates with nx columns and just the rows an edge slice of `rows`
    rows from EDGE_ROW_BEGIN needs."""
    return saddle(nx, EDGE_ROW_BEGIN + rows)


def _edge_class(n: int, unit: int):
    """-1, 0 or +1 when n is one fewer than, exactly or one more than a whole number of
    `unit`s (0 before +1 before -1 where a small unit makes them coincide), else None."""
    r = n % unit
    return 0 if r == 0 else 1 if r == 1 else -1 if r == unit - 1 else None


def own_edge(native, nx: int, rows: int, grid: int):
    """Where (nx, rows) sits in the shape expr2d_shape gives that very launch, or None when
    it is on no edge of it: (lanes along x, columns per lane, column class, row class,
    min(panels, 2), min(stretches, 2)). Column class: nx against whole panels of lanes_x *
    cols_per_lane columns; row class: the longest stretch's rows against whole turns of the
    256 / lanes_x lanes along y (_edge_class)."""
    s = native.expr2d_shape(nx, rows, grid)
    col = _edge_class(nx, s.lanes_x * s.cols_per_lane)
    row = _edge_class(s.rows_per_item, BLOCK // s.lanes_x)
    if col is None or row is None:
        return None
    return s.lanes_x, s.cols_per_lane, col, row, min(s.panels, 2), min(s.stretches, 2)


SHAPE_EDGE_NX, SHAPE_EDGE_ROWS = 1040, 48     # the search box: its corner keeps the budget
_SHAPE_EDGES: dict = {}


def shape_edges(native, grid: int) -> dict:
    """{own_edge signature: the first (nx, rows) of the search box that has it}: launches
    that sit on, one short of or one past a panel and a lane-turn boundary of the shape they
    themselves run with, one for every such place the shape function offers at this cap."""
    if grid not in _SHAPE_EDGES:
        found = {}
        for nx in range(1, SHAPE_EDGE_NX + 1):
            for rows in range(1, SHAPE_EDGE_ROWS + 1):
                sig = own_edge(native, nx, rows, grid)
                if sig is not None:
                    found.setdefault(sig, (nx, rows))
        _SHAPE_EDGES[grid] = found
    return _SHAPE_EDGES[grid]


SLICE_CASE = SADDLE_TALL       # 257 rows = 7 * 36 + 5: ranks 1 .. 5 begin on rows 37, 74, ...


def rank_slices(n: int, world: int = WORLD) -> list:
    return [rank_slice(n, r, world) for r in range(world)]


# the non-exact integrand: exp(-(x*x + y*y)) on [0, 3]^2, 253 x 131 samples (no dyadic step)
GAUSS = (0.0, 3.0, 253, 0.0, 3.0, 131)
# one ulp each for the device's and numpy's exp, and the roundings of x*x + y*y whichever way
# it is contracted: x*x, y*y and the sum round (3 half ulps of an argument below 18, each
# moving exp by at most 18 * 2**-53 of itself), twice (the device's form and numpy's)
GAUSS_C = 2.0 + 2.0 * 3.0 * 18.0 / 2.0


def gauss_reference(rule: str) -> tuple[float, float]:
    """(math.fsum of numpy's exp at coordinates formed in rationals and rounded once, times
    hx * hy in fp64; the sum of |f| times |hx * hy|)."""
    import math
    from fractions import Fraction

    ax, bx, nx, ay, by, ny = GAUSS
    off = Fraction(OFF2[rule], 2)
    hx, hy = (bx - ax) / nx, (by - ay) / ny          # the fp64 steps the kernels use
    xs = np.array([float(Fraction(ax) + (i + off) * Fraction(hx)) for i in range(nx)])
    ys = np.array([float(Fraction(ay) + (j + off) * Fraction(hy)) for j in range(ny)])
    f = np.exp(-(xs[None, :] * xs[None, :] + ys[:, None] * ys[:, None]))
    s = math.fsum(f.reshape(-1).tolist())
    return s * (hx * hy), s * abs(hx * hy)
