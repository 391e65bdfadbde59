"""The exact tests of the run-time expression kernels, the part that needs no GPU: the new
integer references against fractions.Fraction, every case of expr_exact_cases.py within its
exactness budget, the structural facts test_expr_exact_gpu.py leans on (launch shapes, chunk
count, odd slice starts, rows per row lane), and the host twins (HostExpr, HostExprSweep in
csrc/runtime/host_expr.cpp) on the same cases, bit for bit."""
from __future__ import annotations

import math
import random
from fractions import Fraction

import numpy as np
import pytest

import expr_exact_cases as ec
from cuda_v_mpi_amd.utils import exact_riemann as xr


def _x(a_num, k, off2, i) -> Fraction:
    return Fraction(a_num + 2 * i + off2, 1 << (k + 1))


# ------------------------------------------------------------------------------ references
def test_absline_reference_against_fractions():
    rng = random.Random(5)
    for _ in range(300):
        k = rng.choice((0, 2, 7, 10))
        off2 = rng.choice((0, 1, 2))
        a_num = rng.randrange(-16 << (k + 1), 16 << (k + 1))
        p0, p1, p2 = rng.randrange(-16 << (k + 1), 16 << (k + 1)), rng.randrange(-7, 8), rng.randrange(-7, 8)
        i = rng.randrange(0, 1 << 12)
        got = int(xr.exact_absline_samples(p0, p1, p2, a_num, k, off2, i, 1)[0])
        want = p2 + p1 * abs(_x(a_num, k, off2, i) - Fraction(p0, 1 << (k + 1)))
        assert Fraction(got, 1 << (k + 1)) == want, (k, off2, a_num, p0, p1, p2, i)
    at = ec.CUBIC.at
    for p0, p1, p2 in ec.ABS_ROWS:
        tot = xr.exact_absline_sum(p0, p1, p2, at.a_num, at.k, 1, 5, 300)
        want = sum(p2 + p1 * abs(_x(at.a_num, at.k, 1, i) - Fraction(p0, 1 << (at.k + 1)))
                   for i in range(5, 305))
        assert Fraction(tot, 1 << (at.k + 1)) == want


def test_linear_rows_reference_against_fractions():
    for c in ec.LINEAR_CASES:
        rows = ec.linear_rows(c)
        b, m = c.at.span
        for off2 in (0, 1, 2):
            assert xr.sample_moments(c.at.a_num, off2, b, min(m, 300)) == (
                min(m, 300), sum(c.at.a_num + 2 * i + off2 for i in range(b, b + min(m, 300))))
            got = xr.exact_linear_rows_sums(rows, c.at.a_num, c.at.k, off2, b, min(m, 300))
            for r in (0, 1, 2, len(rows) // 2, len(rows) - 1):
                p0, p1 = (int(v) for v in rows[r])
                want = sum(p1 * _x(c.at.a_num, c.at.k, off2, i) + p0 for i in range(b, b + min(m, 300)))
                assert Fraction(int(got[r]), 1 << (c.at.k + 1)) == want, (c.name, off2, r)
                # and the polynomial reference, on the whole slice
                assert int(xr.exact_linear_rows_sums(rows[r:r + 1], c.at.a_num, c.at.k, off2, b, m)[0]) \
                    == xr.exact_poly_sum((p0, p1), c.at.a_num, c.at.k, off2, b, m)


def test_wide_rows_reference_against_fractions():
    """The degree-7 and degree-4 rows: int64 Horner against fractions on all 37 samples."""
    at = ec.WIDE_AT
    for rows in (ec.HORNER8_ROWS, ec.HORNER5_ROWS):
        for coef in rows:
            for off2 in (0, 1, 2):
                want = sum(sum(c * _x(at.a_num, at.k, off2, i) ** j for j, c in enumerate(coef))
                           for i in range(at.n))
                tot = xr.exact_poly_sum(coef, at.a_num, at.k, off2, 0, at.n)
                assert Fraction(tot, 1 << xr.poly_unit_bits(coef, at.k)) == want


def test_values_f64_is_value_f64():
    t = np.array([0, 1, -3, (1 << 53) - 1, -(1 << 52) - 5], dtype=np.int64)
    for u in (0, 1, 11, 40):
        assert ec.bits(xr.values_f64(t, u)) == ec.bits([xr.value_f64(int(v), u) for v in t])
    with pytest.raises(ValueError):
        xr.values_f64(np.array([1 << 53], dtype=np.int64), 3)


def test_expr_budget_by_hand():
    # 3 - 5 x + 7 x^2 at k = 1 (unit 1/16), samples num = -9 .. -9 + 2 * 4 + 2 = 1: |num| <= 9
    assert xr.expr_budget_bits((3, -5, 7), -9, 1, 0, 5) == math.log2(5 * (3 * 16 + 5 * 9 * 4 + 7 * 81))
    # a constant: D = 1; the whole rule's samples when the slice is a rank's share
    assert xr.expr_budget_bits((4,), 0, 2, 3, 2, 0, 100) == math.log2(100 * 4 * 8)
    # |x| < 1 everywhere: max(|num|, 1) keeps the powers from shrinking the bound
    assert xr.expr_budget_bits((0, 0, 1), 0, 3, 0, 1) >= 0.0
    assert xr.absline_budget_bits(-6, -3, 2, -9, 1, 0, 5) == math.log2(5 * (2 * 4 + 3 * (9 + 6)))


# ------------------------------------------------------------------------------ budgets
def _budgets() -> dict:
    out = {c.name: ec.poly_budget(c.coef, c.at) for c in ec.POLY_EXPRS}
    out.update({c.name: ec.linear_budget(c) for c in ec.LINEAR_CASES})
    out["horner8"] = ec.poly_budget(ec.HORNER8_FULL, ec.WIDE_AT)
    return out


def test_every_case_within_budget():
    b = _budgets()
    b["cubic rows"] = ec.rows_budget(ec.CUBIC_ROWS, ec.CUBIC.at)
    b["abs rows"] = ec.abs_budget(ec.ABS_ROWS, ec.CUBIC.at)
    for rows in (20, 7):
        b[f"unequal {rows}"] = ec.rows_budget(ec.unequal_rows(rows), ec.CUBIC.at)
    b["horner8 rows"] = ec.rows_budget(ec.HORNER8_ROWS, ec.WIDE_AT)
    b["horner5 rows"] = ec.rows_budget(ec.HORNER5_ROWS, ec.WIDE_AT)
    for name, v in b.items():
        print(f"{name}: {v:.1f} bits")
        assert v < xr.F64_BITS, name
    for name, v in ec.BUDGETS.items():
        assert round(b[name], 1) == v, name


def test_case_rows_are_what_the_budgets_assume():
    for c in ec.LINEAR_CASES:
        r = ec.linear_rows(c)
        assert r.shape == (c.rows, 2) and int(np.abs(r).max()) == 7
        assert r[:2].tolist() == [[1, 0], [0, 1]] and r[-1].tolist() == r[-2].tolist()
    assert max(abs(v) for r in ec.HORNER8_ROWS + ec.HORNER5_ROWS for v in r) == 3
    assert all(len(r) == 8 for r in ec.HORNER8_ROWS) and all(len(r) == 5 for r in ec.HORNER5_ROWS)
    at = ec.CUBIC.at
    for p0, _, _ in ec.ABS_ROWS:          # every knot inside the domain
        assert at.a_num < p0 < at.a_num + 2 * at.n
    assert {p0 % 2 for p0, _, _ in ec.ABS_ROWS} == {0, 1}   # on left / right and on mid samples
    assert ec.CUBIC_ROWS[:4] == ec.unit_rows(4) and ec.CUBIC_ROWS[4] == ec.CUBIC_ROWS[-1] == ec.CUBIC.coef


def test_coordinates_are_exact_in_fp64():
    """a, b and (b - a) / n = 2**-k: what the kernels are handed is what the reference has."""
    ats = [c.at for c in ec.POLY_EXPRS + ec.LINEAR_CASES] + [ec.WIDE_AT]
    for at in ats:
        assert Fraction(at.a) == Fraction(at.a_num, 1 << (at.k + 1))
        assert Fraction(at.b) == Fraction(at.a) + Fraction(at.n, 1 << at.k)
        assert (at.b - at.a) / float(at.n) == 2.0 ** -at.k


# ------------------------------------------------------------------------------ structure
def test_slices_begin_on_odd_samples():
    begins = [b for b, _ in ec.rank_slices(ec.SLICE_CASE.at.n)]
    assert sum(b % 2 for b in begins) >= 3 and begins[0] == 0
    assert sum(m for _, m in ec.rank_slices(ec.SLICE_CASE.at.n)) == ec.SLICE_CASE.at.n
    assert ec.EDGE_BEGIN % 2 == 1 and ec.PAST_2_32.at.begin % 2 == 1


def test_edge_runs_cover_every_count():
    for grid in (1, 3):
        lanes = ec.BLOCK * grid
        want = {1, 3, 255, 256, 257, lanes - 1, lanes, lanes + 1, 4 * lanes + 3}
        assert {m for _, m in ec.edge_runs(grid)} == want
        assert (4 * lanes + 3) // lanes % 4 == 0 and (4 * lanes + 3) % lanes == 3
    # per-lane counts that are no multiple of 4 at one workgroup
    assert (ec.CUBIC.at.n // ec.BLOCK) % 4 == 0 and ec.CUBIC.at.n % ec.BLOCK != 0
    assert ec.FULL_LANES.at.n == 4 * 2048 * ec.BLOCK + 3


def test_sweep_shapes_and_chunks(native):
    at = ec.CUBIC.at
    for (grid, rows), (gy, per_lane) in ec.UNEQUAL_LANES.items():
        assert native.expr_sweep_shape(at.n, rows, grid) == (grid, gy)
        assert [len(range(by, rows, gy)) for by in range(gy)] == per_lane
        assert max(per_lane) > 2 and len(set(per_lane)) > 1
    c = ec.AUTO_SHAPE
    gx, gy = native.expr_sweep_shape(c.at.n, c.rows)
    assert (gx, gy) == ec.AUTO_SHAPE_GXGY
    assert {len(range(by, c.rows, gy)) for by in range(gy)} == {1, 2}
    c = ec.CHUNKED
    assert native.expr_sweep_shape(c.at.n, c.rows, c.grid) == (2048, 1)
    assert c.rows * c.grid > native.SWEEP_MAX_PARTIALS == 1 << 24
    assert ec.chunk_rows(native, c) == 8192 and c.rows - 8192 == 3
    assert ec.chunk_rows(native, ec.AUTO_SHAPE) == ec.AUTO_SHAPE.rows      # one chunk
    assert native.expr_sweep_shape(ec.PAST_2_32.at.span[1], ec.PAST_2_32.rows) == (1, 9)
    assert max(ec.REUSE_ROWS[1:2]) > max(ec.REUSE_ROWS[0], ec.REUSE_ROWS[2])


# ------------------------------------------------------------------------------ host twins
@pytest.fixture(scope="module")
def pools(native):
    return {t: native.HostPool(t) for t in (1, 3, 4)}


def _host_counts(threads: int) -> list:
    """Slice lengths around the 4096-sample block of every thread's share: one short, whole,
    one over, 8 m + r (the 8-way loop and its tail), and a few samples only."""
    B = ec.HOST_BLOCK
    return [1, 5, 8 * 37 + 5, threads * B - 1, threads * B, threads * B + 1,
            threads * (B + 8 * 3) + 5, 4095, 4096, 4097]


@pytest.mark.parametrize("threads", [1, 3, 4])
def test_host_expr_exact(native, pools, threads):
    c = ec.QUADRATIC
    he = native.HostExpr(c.expr)
    for rule in ec.RULES:
        for m in _host_counts(threads):
            got = he.integrate(c.at.a, c.at.b, c.at.n, getattr(native.Rule, rule), ec.EDGE_BEGIN,
                               m, pools[threads])
            assert got == ec.poly_value(c.coef, c.at, rule, ec.EDGE_BEGIN, m), (rule, m)
    for c in ec.POLY_EXPRS:
        he = native.HostExpr(c.expr)
        for r, (b, m) in enumerate([(0, c.at.n)] + ec.rank_slices(c.at.n)):
            rule = ec.RULES[r % 3]
            got = he.integrate(c.at.a, c.at.b, c.at.n, getattr(native.Rule, rule), b, m,
                               pools[threads])
            assert got == ec.poly_value(c.coef, c.at, rule, b, m), (c.name, r)


def _host_sweep(native, expr, rows, at, rule, begin, count, pool) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.float64)
    return native.HostExprSweep(expr, rows.shape[1]).integrate(
        rows, at.a, at.b, at.n, getattr(native.Rule, rule), begin, count, pool)


@pytest.mark.parametrize("threads", [1, 3, 4])
def test_host_sweep_exact(native, pools, threads):
    pool = pools[threads]
    at = ec.CUBIC.at
    for rule in ec.RULES:
        assert ec.bits(_host_sweep(native, ec.CUBIC_SWEEP, ec.CUBIC_ROWS, at, rule, 0, at.n, pool)) \
            == ec.bits(ec.poly_rows_values(ec.CUBIC_ROWS, at, rule, 0, at.n))
        assert ec.bits(_host_sweep(native, ec.ABS_SWEEP, ec.abs_params(ec.ABS_ROWS, at.k), at, rule,
                                   0, at.n, pool)) == ec.bits(ec.abs_values(ec.ABS_ROWS, at, rule, 0, at.n))
        for expr, rows in ((ec.HORNER8, ec.HORNER8_ROWS), (ec.HORNER5, ec.HORNER5_ROWS)):
            w = ec.WIDE_AT
            assert ec.bits(_host_sweep(native, expr, rows, w, rule, 0, w.n, pool)) \
                == ec.bits(ec.poly_rows_values(rows, w, rule, 0, w.n)), (expr, rule)
    rule = ec.RULES[threads % 3]
    for c in (ec.CHUNKED, ec.PAST_2_32):
        b, m = c.at.span
        assert ec.bits(_host_sweep(native, ec.LINEAR_SWEEP, ec.linear_rows(c), c.at, rule, b, m, pool)) \
            == ec.bits(ec.linear_values(c, rule)), c.name
    # the auto-shape case: 50 of its rows, slices around the host block from an odd sample
    c = ec.AUTO_SHAPE
    rows = ec.linear_rows(c)[:50]
    for m in _host_counts(threads) + [c.at.n - ec.EDGE_BEGIN]:
        tot = xr.exact_linear_rows_sums(rows, c.at.a_num, c.at.k, ec.OFF2[rule], ec.EDGE_BEGIN, m)
        assert ec.bits(_host_sweep(native, ec.LINEAR_SWEEP, rows, c.at, rule, ec.EDGE_BEGIN, m, pool)) \
            == ec.bits(xr.values_f64(tot, c.at.k + 1) * 2.0 ** -c.at.k), m
