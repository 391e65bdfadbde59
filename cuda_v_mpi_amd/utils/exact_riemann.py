"""Exact references of the Riemann-sum and 2-D field kernels, in integers only.

The sibling of exact_scan.py for csrc/kernels/riemann.hip (table and polynomial integrands,
integrands.hpp / integrands_f32.hpp), the 2-D field kernels of csrc/kernels/table.hip and
the run-time expression kernels (csrc/runtime/expr.cpp, expr_sweep.cpp, host_expr.cpp).
With integer table entries or coefficients, a step h = 2**-k and a lower limit a =
a_num / 2**(k+1), every sample coordinate, every sample value and every intermediate any
kernel forms from them (tile midpoints, segment lines, kinks, Taylor shifts, pair sums,
lane, wave and block sums, per-workgroup partials) is a small multiple of one power of two.
While those multiples stay below 2**53 (2**24 for what a packed-fp32 path rounds to fp32)
no operation rounds, in any order, so every path must return the bits of the integer sum.
This module computes that sum in int64 / Python integers, and the budgets that say, from
the inputs alone, whether a case is small enough for the claim to hold.

Coordinates: sample i sits at x = a + (i + off) * 2**-k with off2 = 2 * off in {0, 1, 2}
(left, mid, right), i.e. at num_i = a_num + 2 * i + off2 in units of 2**-(k+1).

    tab = jagged_table(200, 7, seed=3)
    assert table_budget_bits(tab, a_num, k, off2, 0, n, 0, n)["fp64"] < 53
    ref = exact_table_sum(tab, a_num, k, off2, 0, n)        # units of 2**-(k+1)
    value == value_f64(ref, k + 1) * 2.0**-k                  # the kernel's h * sum, bitwise
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .exact_scan import jagged_table, to_f64  # noqa: F401  (re-exported: one place to import)

TILE = 64          # samples per segment-line / Taylor-pair tile (Table::kSeriesTile, Poly's)
F64_BITS = 53
F32_BITS = 24
# Samples one fp32 accumulator adds up before it is folded into fp64: a pair accumulator
# takes the 16 + / - samples of a sub-tile (16), the kIeee tiles 16 per chain; the coarse
# fallback of a 64-sample series tile runs 2 chains of 32 (TableF32::tile_acc), the most.
F32_CHAIN = 32


def _check_coords(k: int, off2: int, i_begin: int, n: int) -> None:
    if k < 0 or off2 not in (0, 1, 2) or i_begin < 0 or n < 1:
        raise ValueError("need k >= 0, off2 in {0, 1, 2}, i_begin >= 0, n >= 1")


def _nums(a_num: int, off2: int, i_begin: int, n: int) -> torch.Tensor:
    return int(a_num) + int(off2) + 2 * torch.arange(i_begin, i_begin + n, dtype=torch.int64)


def _table(table) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(table))
    if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 2:
        raise ValueError("table must be a 1-D int64 array of at least 2 entries")
    return t


def _segments(T: torch.Tensor, num: torch.Tensor, k: int) -> torch.Tensor:
    # floor(x) = num >> (k + 1) (arithmetic shift: floor for negative x too), clamped
    return torch.clamp(num >> (k + 1), 0, T.numel() - 2)


# ------------------------------------------------------------------------------ 1-D table
def exact_table_samples(table, a_num: int, k: int, off2: int, i_begin: int,
                        n: int) -> torch.Tensor:
    """Samples i_begin .. i_begin + n - 1 of the piecewise-linear table (entries at x = 0, 1,
    ...), int64 in units of 2**-(k+1): T[s] * 2**(k+1) + (T[s+1] - T[s]) * (num - s * 2**(k+1))
    with s = clamp(floor(x), 0, entries - 2). Past either end the end segment's line goes on,
    as Table::point has it."""
    _check_coords(k, off2, i_begin, n)
    T = _table(table)
    num = _nums(a_num, off2, i_begin, n)
    s = _segments(T, num, k)
    v0 = T[s]
    return (v0 << (k + 1)) + (T[s + 1] - v0) * (num - (s << (k + 1)))


def exact_table_sum(table, a_num: int, k: int, off2: int, i_begin: int, n: int) -> int:
    """Sum of exact_table_samples (a Python integer, units of 2**-(k+1))."""
    return int(exact_table_samples(table, a_num, k, off2, i_begin, n).sum())


def table_tile_census(table, a_num: int, k: int, off2: int, i_begin: int, n: int) -> dict:
    """How many of the slice's 64-sample tiles take each path of the segment-line tiles
    (Table::tile_acc, TableF32::tile_acc): {"one", "kink", "coarse", "rem"}. The rule is
    Table::ends': the segments lo, hi of samples 0 and 63 of each consecutive tile from
    i_begin; lo == hi is a one-segment line, hi == lo + 1 a kinked line, anything else the
    per-sample fallback. "rem" counts the samples past the last whole tile."""
    _check_coords(k, off2, i_begin, n)
    T = _table(table)
    tiles = n // TILE
    out = {"one": 0, "kink": 0, "coarse": 0, "rem": n - tiles * TILE}
    if tiles:
        first = int(a_num) + int(off2) + 2 * (i_begin + TILE * torch.arange(tiles, dtype=torch.int64))
        lo = _segments(T, first, k)
        hi = _segments(T, first + 2 * (TILE - 1), k)
        out["one"] = int((hi == lo).sum())
        out["kink"] = int((hi == lo + 1).sum())
        out["coarse"] = tiles - out["one"] - out["kink"]
    return out


def table_kink_slope_sums(table, a_num: int, k: int, off2: int, i_begin: int, n: int) -> dict:
    """For the slice's kinked tiles: {knot position inside the tile, in half steps from its
    first sample: sum of the slope changes T[s+1] - 2 T[s] + T[s-1] at those tiles' knots}.

    Why it matters: a kinked tile's sum is linear in its slope change dD with a weight that
    depends only on where the knot falls in the tile, so a wrong weight (a sign, an offset)
    moves the launch's sum by sum_g error(g) * slope_sum(g). Where every tile has its knot
    at the same place (64 h = one segment) the slope changes telescope to last slope minus
    first slope, and a case whose end slopes agree cannot see such a mistake: a case list
    needs some slope sum that is not zero (test_exact_riemann_cpu.py asserts it)."""
    _check_coords(k, off2, i_begin, n)
    T = _table(table)
    tiles = n // TILE
    if not tiles:
        return {}
    first = int(a_num) + int(off2) + 2 * (i_begin + TILE * torch.arange(tiles, dtype=torch.int64))
    lo = _segments(T, first, k)
    hi = _segments(T, first + 2 * (TILE - 1), k)
    kink = hi == lo + 1
    knot = lo[kink] + 1
    where = (knot << (k + 1)) - first[kink]
    dd = T[knot + 1] - 2 * T[knot] + T[knot - 1]
    out: dict = {}
    for w, d in zip(where.tolist(), dd.tolist()):
        out[w] = out.get(w, 0) + d
    return out


def _log2(v: int) -> float:
    return math.log2(v) if v > 0 else 0.0


def table_budget_bits(table, a_num: int, k: int, off2: int, i_begin: int, n: int,
                      whole_begin: int | None = None, whole_n: int | None = None) -> dict:
    """log2 of a bound on every intermediate of a launch over samples [i_begin, i_begin + n),
    in units of 2**-(k+1), from the inputs alone.

    One value a kernel forms (a sample, a tile's midpoint or sub-tile centre value on its
    segment's line, a sample of the kinked line before its kink is added) is at most
    m = max |line through a tile's first segment, anywhere in the tile|
      <= max|sample| + 64 |dD|,   |dD| = 2 max|second difference of the table|
    (a line leaves the interpolant by at most the slope change times the distance past the
    knot, under 64 steps; dD = dd * h is 2 dd units). "fp64": n_total * m bounds every sum of
    such values (n_total: the samples of the whole rule when the slice is one rank's share,
    `whole_begin` / `whole_n`, for the all-reduced value). "fp32": F32_CHAIN * m bounds what a
    packed-fp32 path holds in fp32 (vc, r, Df, dDf, every g, the pair accumulators)."""
    T = _table(table)
    wb = i_begin if whole_begin is None else whole_begin
    wn = n if whole_n is None else whole_n
    smax = 0
    for p0 in range(wb, wb + wn, 1 << 22):
        m = min(1 << 22, wb + wn - p0)
        smax = max(smax, int(exact_table_samples(T, a_num, k, off2, p0, m).abs().max()))
    dd = int((T[2:] - 2 * T[1:-1] + T[:-2]).abs().max()) if T.numel() > 2 else 0
    m = smax + TILE * 2 * dd
    return {"fp64": _log2(wn * m), "fp32": _log2(F32_CHAIN * m)}


# ------------------------------------------------------------------------------ polynomial
def _degree(coef) -> int:
    c = [int(v) for v in coef]
    if any(float(v) != int(v) for v in coef):
        raise ValueError("integer coefficients only")
    d = len(c) - 1
    while d > 0 and c[d] == 0:
        d -= 1
    return d


def poly_unit_bits(coef, k: int) -> int:
    """The reference's unit is 2**-poly_unit_bits: deg * (k + 1), deg the highest power with
    a coefficient that is not zero (appended zeros do not move it), at least 1."""
    return max(1, _degree(coef)) * (k + 1)


def exact_poly_samples(coef, a_num: int, k: int, off2: int, i_begin: int,
                       n: int) -> torch.Tensor:
    """p(x_i) = sum_j c_j x_i**j for integer c_j, int64 in units of 2**-(D (k+1)),
    D = max(deg, 1): sum_j c_j num**j 2**((D - j) (k+1)), by Horner in integers."""
    _check_coords(k, off2, i_begin, n)
    deg, D = _degree(coef), max(1, _degree(coef))
    num = _nums(a_num, off2, i_begin, n)
    # sum_j c_j num^j S^(D-j), S = 2^(k+1): Horner from the top, each step times num, the
    # coefficient scaled to the running unit
    r = torch.full_like(num, int(coef[deg]))
    for j in range(deg - 1, -1, -1):
        r = r * num + (int(coef[j]) << ((deg - j) * (k + 1)))
    return r << ((D - deg) * (k + 1))


def exact_poly_sum(coef, a_num: int, k: int, off2: int, i_begin: int, n: int) -> int:
    return int(exact_poly_samples(coef, a_num, k, off2, i_begin, n).sum())


def poly_budget_bits(coef, a_num: int, k: int, off2: int, i_begin: int, n: int,
                     whole_begin: int | None = None, whole_n: int | None = None) -> dict:
    """log2 of a bound on every intermediate of the polynomial kernels, in units of
    2**-(deg (k+1)), from |c_j| and the largest coordinate alone.

    The Taylor-pair tiles (Poly::shift, Poly::parts) run, on absolute values, here: the
    repeated-Horner shift of cs_i = |c_i| h**i at u up to the farthest sub-tile centre in
    steps, then the even / odd Horner in K = k_j**2 up to 15.5**2 and E + k O. The kIeee tiles'
    Horner in x runs on |x| up to the farthest sample. m is the largest value either forms;
    "fp64" = log2(n_total * m), "fp32" = log2(F32_CHAIN * m) (the b_m, E, O, every sample and
    the pair accumulators of PolyF32). Exact rational arithmetic (integers over 2**(deg (k+1)))."""
    deg = _degree(coef)
    D = max(1, deg)
    unit = D * (k + 1)
    wb = i_begin if whole_begin is None else whole_begin
    wn = n if whole_n is None else whole_n
    first = int(a_num) + off2 + 2 * wb
    last = int(a_num) + off2 + 2 * (wb + wn - 1)
    xmax = max(abs(first), abs(last))                  # |x| in units of 2**-(k+1)
    # sub-tile centres sit 16 steps either side of a tile midpoint, itself within the slice:
    # |u_c| <= |x| / h + 16 steps; in half steps (u has one fraction bit)
    u2 = xmax + 2 * 16 + 2 * TILE
    c = [abs(int(v)) for v in coef[:deg + 1]]
    # everything below is an integer in units of 2**-unit
    # cs_i = c_i h**i = c_i 2**(unit - i k) units; b[i] <- b[i+1] * u + b[i], u = u2 / 2
    b = [c[i] << (unit - i * k) for i in range(deg + 1)]
    m = max(b)
    for lo in range(deg):
        for i in range(deg - 1, lo - 1, -1):
            b[i] = (b[i + 1] * u2 >> 1) + b[i] + 1    # + 1: the shift truncates, keep a bound
            m = max(m, b[i])
    K4 = 31 * 31                                        # (15.5)**2 in quarters
    ev, od = deg & ~1, (deg - 1) | 1 if deg >= 1 else 0
    E = b[ev]
    for e in range(ev - 2, -1, -2):
        E = (E * K4 >> 2) + b[e] + 1
        m = max(m, E)
    O = 0
    if deg >= 1:
        O = b[od]
        for o in range(od - 2, 0, -2):
            O = (O * K4 >> 2) + b[o] + 1
            m = max(m, O)
    m = max(m, E + (31 * O >> 1) + 1)
    # kIeee: r <- r x + c_j
    r = c[deg] << unit
    for j in range(deg - 1, -1, -1):
        r = (r * xmax >> (k + 1)) + (c[j] << unit) + 1
        m = max(m, r)
    return {"fp64": _log2(wn * m), "fp32": _log2(F32_CHAIN * m)}


# ------------------------------------------------------------------------------ expressions
# The run-time expression kernels (csrc/runtime/expr.cpp, expr_sweep.cpp, host_expr.cpp) form
# x = fma(idx, h, a) with an exact fp64 index, evaluate the user's expression and add. For an
# expression that is a polynomial in x with integer coefficients the references are the
# polynomial ones above; the bound below is the one that fits what such an expression does
# (Horner in x, nothing else).
def _num_max(a_num: int, begin: int, n: int) -> int:
    """max |num_i| over samples [begin, begin + n) and all three rules (off2 in {0, 1, 2})."""
    return max(abs(int(a_num) + 2 * begin), abs(int(a_num) + 2 * (begin + n - 1) + 2))


def expr_budget_bits(coef, a_num: int, k: int, i_begin: int, n: int,
                     whole_begin: int | None = None, whole_n: int | None = None) -> float:
    """log2 of whole_n * max_i sum_j |c_j| max(|num_i|, 1)**j 2**((D - j) (k+1)), D = max(deg, 1),
    over the samples of the whole rule (default: the slice) and any of the three rules.

    A Horner step r <- r x + c_j on x = num / 2**(k+1) holds, in its own unit 2**-((deg-j)(k+1)),
    at most sum_{i >= j} |c_i| |num|**(i-j) 2**((deg-i)(k+1)), which is no more than the sum
    above (every term only gains factors max(|num|, 1) >= 1 and 2**(k+1) >= 1); the product
    r x before c_j is added, and a step written with or without an fma, likewise. So the sum
    bounds every intermediate of a sample in that intermediate's own unit, and whole_n times
    it every partial sum of samples, in any order, of one launch or of all ranks together.
    Sufficient, not tight. For sweep rows pass the element-wise largest |c_j| of the rows."""
    _check_coords(k, 0, i_begin, n)
    c = [abs(int(v)) for v in coef]
    if any(float(v) != int(v) for v in coef):
        raise ValueError("integer coefficients only")
    deg = len(c) - 1
    while deg > 0 and c[deg] == 0:
        deg -= 1
    D = max(deg, 1)
    wb = i_begin if whole_begin is None else whole_begin
    wn = n if whole_n is None else whole_n
    x = max(_num_max(a_num, wb, wn), 1)
    m = sum(c[j] * x ** j << ((D - j) * (k + 1)) for j in range(deg + 1))
    return _log2(wn * m)


def exact_absline_samples(p0_num: int, p1: int, p2: int, a_num: int, k: int, off2: int,
                          i_begin: int, n: int) -> torch.Tensor:
    """p2 + p1 |x_i - p0| with integer p1, p2 and the knot p0 = p0_num / 2**(k+1): int64 in
    units of 2**-(k+1), p2 2**(k+1) + p1 |num_i - p0_num|. Not a polynomial: a sample that
    sits one place off moves the sum by p1 units on one side of the knot and by -p1 on the
    other, so a coordinate error cannot cancel as it can against a smooth integrand."""
    _check_coords(k, off2, i_begin, n)
    num = _nums(a_num, off2, i_begin, n)
    return (int(p2) << (k + 1)) + int(p1) * (num - int(p0_num)).abs()


def exact_absline_sum(p0_num: int, p1: int, p2: int, a_num: int, k: int, off2: int,
                      i_begin: int, n: int) -> int:
    return int(exact_absline_samples(p0_num, p1, p2, a_num, k, off2, i_begin, n).sum())


def absline_budget_bits(p0_num: int, p1: int, p2: int, a_num: int, k: int, i_begin: int, n: int,
                        whole_begin: int | None = None, whole_n: int | None = None) -> float:
    """The analogue of expr_budget_bits for p2 + p1 fabs(x - p0), in units of 2**-(k+1):
    log2 of whole_n * (|p2| 2**(k+1) + max(|p1|, 1) (max_i |num_i| + |p0_num|)). x, p0, x - p0,
    its absolute value, p1 times it and that plus p2 are each at most the bracket."""
    _check_coords(k, 0, i_begin, n)
    wb = i_begin if whole_begin is None else whole_begin
    wn = n if whole_n is None else whole_n
    m = (abs(int(p2)) << (k + 1)) + max(abs(int(p1)), 1) * (_num_max(a_num, wb, wn) + abs(int(p0_num)))
    return _log2(wn * m)


def sample_moments(a_num: int, off2: int, i_begin: int, n: int) -> tuple[int, int]:
    """(n, sum_i num_i) of samples [i_begin, i_begin + n), Python integers in closed form:
    sum_i (a_num + off2 + 2 i) = n (a_num + off2) + 2 n i_begin + n (n - 1)."""
    _check_coords(0, off2, i_begin, n)
    return n, n * (int(a_num) + int(off2)) + 2 * n * i_begin + n * (n - 1)


def exact_linear_rows_sums(rows, a_num: int, k: int, off2: int, i_begin: int,
                           n: int) -> np.ndarray:
    """Sums of many linear rows at once: row (p0, p1) is f(x) = p1 x + p0, and its samples
    add up to p1 sum_i num_i + p0 n 2**(k+1) in units of 2**-(k+1). `rows` is K x 2 integers;
    the two moments are taken once (sample_moments), the K sums are one int64 expression."""
    _check_coords(k, off2, i_begin, n)
    r = np.asarray(rows)
    if r.ndim != 2 or r.shape[1] != 2 or r.dtype.kind not in "iu":
        raise ValueError("rows must be a K x 2 integer array of (p0, p1)")
    r = r.astype(np.int64)
    s0, s1 = sample_moments(a_num, off2, i_begin, n)
    s0 <<= k + 1
    pmax = int(np.abs(r).max()) if r.size else 0
    if pmax * (abs(s0) + abs(s1)) >= 1 << 62:
        raise ValueError("row sums past int64: no admissible case")
    return r[:, 1] * np.int64(s1) + r[:, 0] * np.int64(s0)


def values_f64(totals, unit_bits: int) -> np.ndarray:
    """value_f64 of an int64 array (every entry below 2**53 in magnitude)."""
    t = np.asarray(totals, dtype=np.int64)
    if t.size and int(np.abs(t).max()) >= 1 << F64_BITS:
        raise ValueError("a reference sum is past 2**53: no admissible case")
    return np.ldexp(t.astype(np.float64), -int(unit_bits))


# ------------------------------------------------------------------------------ 2-D field
def _axis(n_entries: int, rate: tuple, idx: torch.Tensor):
    """Midpoint samples at `rate` = (d, k) table cells per sample (d / 2**k): sample j sits at
    (2 j + 1) d in units of 2**-(k+1). Returns (cell, fraction numerator in those units)."""
    d, k = rate
    num = (2 * idx + 1) * int(d)
    cell = torch.clamp(num >> (k + 1), 0, n_entries - 2)
    return cell, num - (cell << (k + 1))


def table2d_grid_of(n_entries: int, rate: tuple) -> int:
    """Samples along an axis of `n_entries` table entries at `rate` = (d, k) cells per sample
    over the extent n_entries - 1: (n_entries - 1) 2**k / d, which must be whole (then the
    kernel's spacing X / g is d / 2**k exactly)."""
    d, k = rate
    q, r = divmod((n_entries - 1) << k, int(d))
    if r or q < 1:
        raise ValueError(f"rate {d}/2**{k} does not divide {n_entries - 1} table cells")
    return q


def exact_table2d_sum(T, rx: tuple, ry: tuple, gx: int, gy: int, row0: int, row1: int) -> int:
    """Sum over sample rows [row0, row1) and all gx columns of the bilinear interpolant of
    the integer ny x nx table `T`, in units of 2**-(kx + ky + 2) (a Python integer):
    top = v00 2**(kx+1) + (v01 - v00) fx, bot likewise on the next table row,
    value = top 2**(ky+1) + (bot - top) fy. The integral is this sum times sx sy."""
    T = torch.as_tensor(np.asarray(T))
    if T.dtype != torch.int64 or T.dim() != 2 or min(T.shape) < 2:
        raise ValueError("T must be a 2-D int64 array of at least 2 x 2 entries")
    if not 0 <= row0 < row1 <= gy or gx < 1:
        raise ValueError("need 0 <= row0 < row1 <= gy and gx >= 1")
    ny, nx = T.shape
    ix, fx = _axis(nx, rx, torch.arange(gx, dtype=torch.int64))
    total = 0
    for r in range(row0, row1, 512):
        iy, fy = _axis(ny, ry, torch.arange(r, min(r + 512, row1), dtype=torch.int64))
        lo, hi = T[iy], T[iy + 1]
        top = (lo[:, ix] << (rx[1] + 1)) + (lo[:, ix + 1] - lo[:, ix]) * fx
        bot = (hi[:, ix] << (rx[1] + 1)) + (hi[:, ix + 1] - hi[:, ix]) * fx
        total += int(((top << (ry[1] + 1)) + (bot - top) * fy.unsqueeze(1)).sum())
    return total


def table2d_budget_bits(T, rx: tuple, ry: tuple, gx: int, gy: int) -> float:
    """log2 of gx gy max|T| 2**(kx + ky + 2) dx dy: the whole grid's samples, each at most
    max|T| (an interpolant stays inside its corners; the extent ends on the last entry, so no
    sample extrapolates), in units of 2**-(kx + ky + 2), times the numerator of sx sy =
    dx dy / 2**(kx + ky) every workgroup's partial is multiplied by."""
    T = torch.as_tensor(np.asarray(T))
    amax = int(T.abs().max())
    return _log2(gx * gy * amax * (1 << (rx[1] + ry[1] + 2)) * int(rx[0]) * int(ry[0]))


# ------------------------------------------------------------------------------ conversion
def value_f64(total: int, unit_bits: int) -> float:
    """total / 2**unit_bits as an fp64 (exact below 2**53: the budget's promise)."""
    if abs(int(total)) >= 1 << F64_BITS:
        raise ValueError("the reference sum itself is past 2**53: no admissible case")
    return float(to_f64(torch.tensor(int(total), dtype=torch.int64), unit_bits))
