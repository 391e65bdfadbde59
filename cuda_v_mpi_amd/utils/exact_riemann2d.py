"""Exact references of the 2-D run-time expression kernels (csrc/runtime/expr2d.cpp,
HostExpr2D), in integers only: the sibling of exact_riemann.py for f(x, y).

Per axis the coordinates are exact_riemann.py's: a step 2**-k and a lower limit a_num /
2**(k+1), so sample i of the axis sits at num_i = a_num + 2 i + off2 in units of 2**-(k+1)
(off2 = 0, 1, 2 for left, mid, right; the same rule on both axes). With integer coefficients
nothing a kernel forms from such samples rounds while the budget stays below 2**53, in any
order, so every value must have the bits of the integer sum.

    ax = Axis(k=5, a_num=a_num_R(5, 8), n=1025)
    ay = Axis(k=4, a_num=a_num_R(4, 4), n=37)
    assert expr2d_budget_bits(c, ax, ay) < 53
    tot = exact_poly2d_sum(c, ax, ay, off2, row_begin, row_count)    # a Python integer
    value == value_f64(tot, poly2d_unit_bits(c, ax, ay)) * 2.0**-(ax.k + ay.k)   # bitwise
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from .exact_riemann import value_f64  # noqa: F401  (re-exported: one place to import)


class Axis(NamedTuple):
    """One axis of a rule: n samples of step 2**-k from a = a_num / 2**(k+1). A negative step
    (b < a) is `reverse`: sample i then sits at num_i = a_num - 2 i - off2."""
    k: int
    a_num: int
    n: int
    reverse: bool = False

    @property
    def a(self) -> float:
        return self.a_num * 2.0 ** -(self.k + 1)

    @property
    def b(self) -> float:
        return self.a + (-self.n if self.reverse else self.n) * 2.0 ** -self.k

    @property
    def h(self) -> float:
        return (-1.0 if self.reverse else 1.0) * 2.0 ** -self.k


def _check(ax: Axis, off2: int) -> None:
    if ax.k < 0 or ax.n < 1 or off2 not in (0, 1, 2):
        raise ValueError("need k >= 0, n >= 1, off2 in {0, 1, 2}")


def num_of(ax: Axis, off2: int, i: int) -> int:
    """Numerator of sample i of the axis, in units of 2**-(k+1)."""
    step = 2 * int(i) + int(off2)
    return int(ax.a_num) - step if ax.reverse else int(ax.a_num) + step


def power_sum(ax: Axis, off2: int, begin: int, count: int, p: int) -> int:
    """sum over samples [begin, begin + count) of num_i**p, a Python integer: closed form for
    p <= 1 (so a 2**40-sample axis costs nothing), Python integers over chunks of the samples
    for higher powers."""
    _check(ax, off2)
    if count == 0:
        return 0
    first, last = num_of(ax, off2, begin), num_of(ax, off2, begin + count - 1)
    if p == 0:
        return int(count)
    if p == 1:
        return (first + last) * int(count) // 2
    total = 0
    sign = -2 if ax.reverse else 2
    for c0 in range(0, count, 1 << 16):
        m = min(1 << 16, count - c0)
        nums = (first + sign * c0) + sign * np.arange(m, dtype=np.int64)
        total += int((nums.astype(object) ** p).sum())
    return total


def _terms(coef: dict) -> dict:
    out = {}
    for (p, q), c in coef.items():
        if float(c) != int(c) or p < 0 or q < 0:
            raise ValueError("integer coefficients on powers >= 0 only")
        if int(c):
            out[(int(p), int(q))] = int(c)
    if not out:
        out[(0, 0)] = 0
    return out


def poly2d_degrees(coef: dict) -> tuple[int, int]:
    """(dx, dy): the highest powers of x and of y with a coefficient that is not zero, each
    at least 1 (as exact_riemann.poly_unit_bits keeps the unit of a constant)."""
    t = _terms(coef)
    return max(1, max(p for p, _ in t)), max(1, max(q for _, q in t))


def poly2d_unit_bits(coef: dict, ax: Axis, ay: Axis) -> int:
    """The reference's unit is 2**-(dx (kx+1) + dy (ky+1))."""
    dx, dy = poly2d_degrees(coef)
    return dx * (ax.k + 1) + dy * (ay.k + 1)


def exact_poly2d_sum(coef: dict, ax: Axis, ay: Axis, off2: int, row_begin: int,
                     row_count: int) -> int:
    """sum over all ax.n columns and rows [row_begin, row_begin + row_count) of
    sum_pq c_pq x**p y**q for integer c[(p, q)], a Python integer in units of
    2**-(dx (kx+1) + dy (ky+1)): sum_pq c_pq (sum_i num_i**p) (sum_j num_j**q)
    2**((dx - p)(kx+1) + (dy - q)(ky+1)), the two moments in Python integers."""
    if not (0 <= row_begin and row_begin + row_count <= ay.n):
        raise ValueError("rows outside [0, ny)")
    t = _terms(coef)
    dx, dy = poly2d_degrees(coef)
    sx = {p: power_sum(ax, off2, 0, ax.n, p) for p in {p for p, _ in t}}
    sy = {q: power_sum(ay, off2, row_begin, row_count, q) for q in {q for _, q in t}}
    return sum(c * sx[p] * sy[q] << ((dx - p) * (ax.k + 1) + (dy - q) * (ay.k + 1))
               for (p, q), c in t.items())


def _num_max(ax: Axis, begin: int = 0, count: int | None = None) -> int:
    """max(|num_i|, 1) over samples [begin, begin + count) of the axis (default: all of them)
    and all three rules."""
    count = ax.n - begin if count is None else count
    return max(abs(num_of(ax, 0, begin)), abs(num_of(ax, 2, begin + count - 1)), 1)


def _log2(v: int) -> float:
    return math.log2(v) if v > 0 else 0.0


def expr2d_budget_bits(coef: dict, ax: Axis, ay: Axis, row_begin: int = 0,
                       row_count: int | None = None) -> float:
    """log2 of samples * sum_pq |c_pq| max(|xnum|, 1)**p max(|ynum|, 1)**q
    2**((dx - p)(kx+1) + (dy - q)(ky+1)) over the whole rule and any of the three rules (or
    over rows [row_begin, row_begin + row_count) when only that slice is ever summed).

    exact_riemann.expr_budget_bits's argument, taken per term: whatever an expression that
    is this polynomial forms on the way to a sample (a Horner step in x whose coefficients are
    polynomials in y, a product x**p y**q, with or without an fma) is, in its own unit, at
    most the sum of the absolute terms it is made of, each of which only gains factors
    max(|num|, 1) >= 1 and 2**(k+1) >= 1 on the way to the sum above. So the sum bounds every
    intermediate of a sample, and nx ny times it every partial sum of samples, in any order,
    of one launch or of all ranks together. Sufficient, not tight."""
    t = _terms(coef)
    dx, dy = poly2d_degrees(coef)
    rows = ay.n - row_begin if row_count is None else row_count
    xm, ym = _num_max(ax), _num_max(ay, row_begin, rows)
    m = sum(abs(c) * xm ** p * ym ** q << ((dx - p) * (ax.k + 1) + (dy - q) * (ay.k + 1))
            for (p, q), c in t.items())
    return _log2(ax.n * rows * m)


def _grid(ax: Axis, ay: Axis, off2: int, row_begin: int, row_count: int):
    if ax.k != ay.k:
        raise ValueError("the int64 grid references want kx == ky (one unit for x - y)")
    if ax.n * row_count > 1 << 24:
        raise ValueError("the int64 grid references are for small grids")
    sx, sy = (-2 if ax.reverse else 2), (-2 if ay.reverse else 2)
    xn = num_of(ax, off2, 0) + sx * np.arange(ax.n, dtype=np.int64)
    yn = num_of(ay, off2, row_begin) + sy * np.arange(row_count, dtype=np.int64)
    return xn[None, :], yn[:, None]


def exact_absdiff_sum(p1: int, p2: int, ax: Axis, ay: Axis, off2: int, row_begin: int,
                      row_count: int) -> int:
    """sum of p1 |x - y| + p2 over the slice for integer p1, p2 and kx == ky = k, in units
    of 2**-(k+1): p1 |xnum - ynum| + p2 2**(k+1) per sample, an int64 numpy broadcast. The
    kink lies on the diagonal, which no axis owns: a coordinate one place off on either axis
    moves a sample by p1 units up on one side and down on the other and cannot cancel."""
    xn, yn = _grid(ax, ay, off2, row_begin, row_count)
    return int((int(p1) * np.abs(xn - yn) + (int(p2) << (ax.k + 1))).sum())


def absdiff_budget_bits(p1: int, p2: int, ax: Axis, ay: Axis) -> float:
    """log2 of nx ny (max(|p1|, 1) (max|xnum| + max|ynum|) + |p2| 2**(k+1)), units of
    2**-(k+1): x, y, x - y, its absolute value, p1 times it and that plus p2 are each at most
    the bracket."""
    m = max(abs(int(p1)), 1) * (_num_max(ax) + _num_max(ay)) + (abs(int(p2)) << (ax.k + 1))
    return _log2(ax.n * ay.n * m)


def exact_disc_count(r2_num: int, ax: Axis, ay: Axis, off2: int, row_begin: int,
                     row_count: int) -> int:
    """How many samples of the slice have x**2 + y**2 < r2_num / 2**(2 (k+1)) (kx == ky = k):
    the lattice-point count xnum**2 + ynum**2 < r2_num, an int64 numpy broadcast. Every
    sample counts once, at its own place."""
    xn, yn = _grid(ax, ay, off2, row_begin, row_count)
    return int((xn * xn + yn * yn < int(r2_num)).sum())


def disc_budget_bits(ax: Axis, ay: Axis) -> float:
    """log2 of the larger of max (xnum**2 + ynum**2) (what a sample forms, units of
    2**-(2 (k+1))) and nx ny (the count)."""
    return _log2(max(_num_max(ax) ** 2 + _num_max(ay) ** 2, ax.n * ay.n))
