"""The inputs of the exact tests of the run-time expression kernels, in one place:
test_expr_exact_gpu.py launches them on the device (ExprIntegrator, ExprSweep),
test_expr_exact_cpu.py asserts on any box that every one of them keeps its exactness budget
(exact_riemann.expr_budget_bits / absline_budget_bits) and the structural facts the GPU tests
lean on, and runs the host twins (HostExpr, HostExprSweep) on them.

Coordinates as in riemann_exact_cases.py: h = 2**-k, a = -2.625 - 5 h (or -R - 1/8 - 5 h), so
that no lane run starts on a round number, b = a + n h. Every expression is a polynomial in x
with integer coefficients, or p2 + p1 * fabs(x - p0) with a dyadic knot: nothing any kernel
forms from them can round, so every value must have the bits of the integer sum.
"""
from __future__ import annotations

import functools
import gc
from typing import NamedTuple

import numpy as np

from cuda_v_mpi_amd.parallel.decomposition import rank_slice
from cuda_v_mpi_amd.utils import exact_riemann as xr

OFF2 = {"left": 0, "mid": 1, "right": 2}
RULES = ("left", "mid", "right")
WORLD = 7                      # rank slices: rank_slice(n, r, 7)
LOOPBACK_WORLDS = (2, 3)
BLOCK = 256                    # threads of a workgroup of every expression kernel
HOST_BLOCK = 4096              # samples of one compensated block of the host twins


class Coords(NamedTuple):
    """An n-sample rule of step 2**-k from a = a_num / 2**(k+1); `begin`, `count`: the slice
    that is launched and that bounds the budget (the whole rule unless given)."""
    k: int
    a_num: int
    n: int
    begin: int = 0
    count: int | None = None

    @property
    def a(self) -> float:
        return self.a_num * 2.0 ** -(self.k + 1)

    @property
    def b(self) -> float:
        return self.a + self.n * 2.0 ** -self.k

    @property
    def span(self) -> tuple[int, int]:
        return self.begin, self.n - self.begin if self.count is None else self.count


def a_num_of(k: int) -> int:
    """a = -2.625 - 5 h in units of 2**-(k+1) (k >= 2: 2.625 = 21 / 8)."""
    return -(21 << (k - 2)) - 10


def a_num_R(k: int, R: int) -> int:
    """a = -R - 1/8 - 5 h in units of 2**-(k+1)."""
    return -(R << (k + 1)) - (1 << (k - 2)) - 10


# ------------------------------------------------------------------------------ one expression
class PolyExpr(NamedTuple):
    name: str
    expr: str            # what the kernels compile
    coef: tuple          # the same polynomial, c_0 first
    at: Coords


CUBIC = PolyExpr("cubic", "((5.0*x-3.0)*x+7.0)*x-6.0", (-6, 7, -3, 5),
                 Coords(7, a_num_R(7, 8), (16 << 7) + 37))
QUADRATIC = PolyExpr("quadratic", "(7.0*x-5.0)*x+3.0", (3, -5, 7),
                     Coords(10, a_num_R(10, 16), (32 << 10) + 37))
# 2048 workgroups = 524 288 lanes: every lane has 4 samples, the first three have 5
FULL_LANES = PolyExpr("full-lanes", "5.0-7.0*x", (5, -7),
                      Coords(12, a_num_of(12), 4 * 524_288 + 3))
POLY_EXPRS = (CUBIC, QUADRATIC, FULL_LANES)
EXPR_GRIDS = (1, 3, 2048)


def poly_value(coef, at: Coords, rule: str, begin: int, count: int, scale: float = 1.0) -> float:
    """h * scale * sum over samples [begin, begin + count), exactly: the fp64 every launch of
    the case must return (scale a power of two)."""
    tot = xr.exact_poly_sum(coef, at.a_num, at.k, OFF2[rule], begin, count)
    return xr.value_f64(tot, xr.poly_unit_bits(coef, at.k)) * 2.0 ** -at.k * scale


def poly_budget(coef, at: Coords) -> float:
    b, c = at.span
    return xr.expr_budget_bits(coef, at.a_num, at.k, b, c, b, c)


def edge_counts(grid: int) -> list:
    """n_local values that walk the edges of the balanced lane split of `grid` workgroups:
    fewer samples than lanes, a wave's worth either side, the lane count and its neighbours
    (the remainder lanes: all but one, none, one), and 4 per lane plus 3 (the unrolled loop
    once, then the remainder loop on three lanes)."""
    lanes = BLOCK * grid
    return sorted({1, 3, 255, 256, 257, lanes - 1, lanes, lanes + 1, 4 * lanes + 3})


EDGE_BEGIN = 5       # an odd first sample for every edge slice


def edge_runs(grid: int) -> list:
    """(case, n_local) for every edge count at `grid`: on the cubic where the slice
    [EDGE_BEGIN, EDGE_BEGIN + n_local) fits its 2085 samples, on the quadratic too (it holds
    them all, 4 * 768 + 3 included)."""
    out = []
    for m in edge_counts(grid):
        out += [(c, m) for c in (CUBIC, QUADRATIC) if EDGE_BEGIN + m <= c.at.n]
    return out


SLICE_CASE = QUADRATIC     # 32 805 = 7 * 4686 + 3: ranks 1, 3, 4, 5, 6 begin on odd samples


def rank_slices(n: int, world: int = WORLD) -> list:
    return [rank_slice(n, r, world) for r in range(world)]


# ------------------------------------------------------------------------------ sweeps
CUBIC_SWEEP = "p0+x*(p1+x*(p2+x*p3))"                       # 4 parameters
ABS_SWEEP = "p2+p1*fabs(x-p0)"                               # 3 parameters
LINEAR_SWEEP = "p1*x+p0"                                     # 2 parameters
HORNER5 = "p0+x*(p1+x*(p2+x*(p3+x*p4)))"
HORNER8 = "p0+x*(p1+x*(p2+x*(p3+x*(p4+x*(p5+x*(p6+x*p7))))))"
SWEEP_GRIDS = (1, 2, 7, 0)     # 0: the auto shape


def unit_rows(width: int) -> list:
    return [tuple(int(i == j) for i in range(width)) for j in range(width)]


# the unit vectors pin the moments sum 1, sum x, sum x^2, sum x^3 of the sample set one by
# one; then the cubic itself, a second vector, and the cubic once more (a repeated row)
CUBIC_ROWS = unit_rows(4) + [CUBIC.coef, (2, 0, -7, 1), CUBIC.coef]

# (p0_num, p1, p2): the knot in units of 2**-(k+1) of the cubic's coordinates (k = 7, samples
# at even numerators for left / right and odd ones for mid, from -2090 to 2080). Knots on a
# left sample, on a midpoint, near both ends, and slope 0 (the plain count of samples).
ABS_ROWS = [(-78, 3, -5), (-77, 3, -5), (512, -2, 7), (1001, 1, 0), (-2085, 5, 1),
            (2071, -4, -3), (0, 0, 1), (512, -2, 7)]


def abs_params(rows, k: int) -> list:
    """The rows as the kernel's p0, p1, p2 (p0 as a coordinate)."""
    return [[p0 * 2.0 ** -(k + 1), float(p1), float(p2)] for p0, p1, p2 in rows]


def abs_values(rows, at: Coords, rule: str, begin: int, count: int, scale: float = 1.0) -> list:
    return [xr.value_f64(xr.exact_absline_sum(p0, p1, p2, at.a_num, at.k, OFF2[rule], begin,
                                              count), at.k + 1) * 2.0 ** -at.k * scale
            for p0, p1, p2 in rows]


def abs_budget(rows, at: Coords) -> float:
    b, c = at.span
    return max(xr.absline_budget_bits(p0, p1, p2, at.a_num, at.k, b, c, b, c)
               for p0, p1, p2 in rows)


def poly_rows_values(rows, at: Coords, rule: str, begin: int, count: int,
                     scale: float = 1.0) -> list:
    """Each row against its own reference (its own degree, so its own unit)."""
    return [poly_value(r, at, rule, begin, count, scale) for r in rows]


def rows_budget(rows, at: Coords) -> float:
    """The budget of the element-wise largest |c_j| of the rows: it bounds every row's."""
    return poly_budget(tuple(int(v) for v in np.abs(np.asarray(rows)).max(axis=0)), at)


@functools.lru_cache(maxsize=None)
def random_rows(count: int, width: int, cmax: int, seed: int):
    """count x width integers in [-cmax, cmax] (a read-only array)."""
    r = np.random.default_rng(seed).integers(-cmax, cmax + 1, size=(count, width), dtype=np.int64)
    r.setflags(write=False)
    return r


# row lanes with unequal work, on the cubic's coordinates: (grid, rows) -> gy and the rows
# each row lane takes (asserted in test_expr_exact_cpu.py)
UNEQUAL_LANES = {(300, 20): (6, [4, 4, 3, 3, 3, 3]), (1024, 7): (2, [4, 3])}


def unequal_rows(rows: int):
    return random_rows(rows, 4, 7, seed=rows)


# degree-7 Horner, |c| <= 3, k = 2 and 37 samples on [-3.875, 5.375]; and five parameters
WIDE_AT = Coords(2, a_num_of(2), 37)
HORNER8_FULL = (-1, 3, -2, 1, -3, 2, -1, 3)
HORNER8_ROWS = unit_rows(8) + [HORNER8_FULL, (3, -3, 3, -3, 3, -3, 3, -3), HORNER8_FULL]
HORNER5_FULL = (2, -3, 1, 3, -2)
HORNER5_ROWS = unit_rows(5) + [HORNER5_FULL, (-3, 3, 3, -3, 1), HORNER5_FULL]


class LinearCase(NamedTuple):
    name: str
    rows: int
    grid: int            # 0: auto
    at: Coords
    seed: int


AUTO_SHAPE = LinearCase("auto-gx3", 1000, 0, Coords(10, a_num_of(10), 131_073), 3)
AUTO_SHAPE_GXGY = (3, 682)      # 318 row lanes take two rows, 364 take one
CHUNKED = LinearCase("chunked", 8195, 2048, Coords(6, a_num_of(6), 1003), 6)
# samples 2^33 + 1 .. 2^33 + 1025 of the 2^40-sample rule of step 1 on [0, 2^40]
PAST_2_32 = LinearCase("past-2^32", 9, 0, Coords(0, 0, 2**40, 2**33 + 1, 1025), 33)
LINEAR_CASES = (AUTO_SHAPE, CHUNKED, PAST_2_32)


def linear_rows(c: LinearCase):
    """K x 2 integers (p0, p1) in [-7, 7]; the first rows are the unit vectors (sum 1 and
    sum x on their own) and (7, -7), the last row repeats the one before."""
    r = random_rows(c.rows, 2, 7, c.seed).copy()
    r[:3] = [(1, 0), (0, 1), (7, -7)]
    r[-1] = r[-2]
    r.setflags(write=False)
    return r


def linear_values(c: LinearCase, rule: str, begin: int | None = None, count: int | None = None,
                  scale: float = 1.0) -> np.ndarray:
    b, m = c.at.span
    b, m = (b if begin is None else begin), (m if count is None else count)
    tot = xr.exact_linear_rows_sums(linear_rows(c), c.at.a_num, c.at.k, OFF2[rule], b, m)
    return xr.values_f64(tot, c.at.k + 1) * 2.0 ** -c.at.k * scale


def linear_budget(c: LinearCase) -> float:
    return poly_budget((7, 7), c.at)


def chunk_rows(native, c: LinearCase) -> int:
    """Rows per chunk of ExprSweep::enqueue for the case's launch shape."""
    gx, _ = native.expr_sweep_shape(c.at.span[1], c.rows, c.grid)
    return min(c.rows, max(native.SWEEP_MAX_PARTIALS // gx, 1))


# one ExprSweep object across small, large, small: the buffers grow and are kept
REUSE_ROWS = (3, 700, 5)

# the budgets of the cases as first computed (bits, one decimal): the CPU test asserts the
# bound itself (< 53) and that none of these moved
BUDGETS = {"cubic": 46.6, "quadratic": 47.9, "full-lanes": 45.8, "horner8": 44.9,
           "auto-gx3": 37.8, "chunked": 23.6, "past-2^32": 46.8}


def bits(v) -> list:
    return np.asarray(v, dtype=np.float64).reshape(-1).view(np.uint64).tolist()


def check_module_lifetime(make, check) -> None:
    """The lifetime of a family's loaded module: objects A and B for one expression (B's
    compile is a cache hit) each own their module, so B still runs after A is destroyed, and
    a fresh C after that. make() builds an object, check(obj, what) asserts one exact launch."""
    a, b = make(), make()
    check(a, "A")
    check(b, "B")
    del a
    gc.collect()
    check(b, "B after A is gone")
    check(make(), "C")
