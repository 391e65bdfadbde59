"""Exact tests of the run-time expression kernels (csrc/runtime/expr.cpp, expr_sweep.cpp):
every value ExprIntegrator and ExprSweep return is compared bit for bit with an integer
reference, no tolerance.

The expressions are polynomials in x with integer coefficients (and p2 + p1 * fabs(x - p0)
with a dyadic knot), h = 2**-k and a dyadic lower limit, so the exact fp64 index, x =
fma(idx, h, a), every Horner step, the four accumulators, the wave and workgroup sums, the
partials and the close are small multiples of one power of two: nothing rounds in any order
(cuda_v_mpi_amd/utils/exact_riemann.py), and every grid, every slice's own reference, every
rank after an all-reduce must have the bits of the integer sum. A dropped or doubled sample
at an edge of the lane split, a row read with the wrong stride, a chunk written over another,
a stale LDS slot of the row loop: each moves a value by at least one unit and fails here,
where the tolerance tests (test_expr_gpu.py, test_expr_sweep_gpu.py) cannot see it.

The inputs live in expr_exact_cases.py; test_expr_exact_cpu.py shows on any box that each
keeps its budget, so a mismatch here is a kernel finding, never an input problem.
"""
from __future__ import annotations

import numpy as np
import pytest

import expr_exact_cases as ec
from cuda_v_mpi_amd.ops import kernels
from cuda_v_mpi_amd.parallel import loopback

pytestmark = pytest.mark.gpu


def _same(got, want, what: str) -> None:
    """Bitwise equality of two fp64 vectors; prints the first rows that differ."""
    g, w = ec.bits(got), ec.bits(want)
    bad = [i for i, (x, y) in enumerate(zip(g, w)) if x != y]
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    print(f"{what}: {len(w)} values, {len(bad)} differ"
          + "".join(f"\n  [{i}] got {got[i]!r} want {want[i]!r}" for i in bad[:8]))
    assert len(g) == len(w) and not bad, what


# ------------------------------------------------------------------------------ one expression
@pytest.fixture(scope="module")
def integrator(native, cuda):
    made = {}

    def get(expr: str, grid: int):
        if (expr, grid) not in made:
            made[expr, grid] = native.ExprIntegrator(expr, cuda.index, grid)
        return made[expr, grid]
    return get


def _one(native, ei, c, rule, begin, count, scale=1.0, comm=None) -> float:
    return ei.integrate(c.at.a, c.at.b, c.at.n, getattr(native.Rule, rule), begin, count, scale,
                        comm)


@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("grid", ec.EXPR_GRIDS)
def test_expr_whole_rule_exact(native, integrator, grid, rule):
    """The cubic and the quadratic, whole, at 1, 3 and 2048 workgroups: 2085 samples are
    fewer than 2048 * 256 lanes, 32 805 leave most lanes empty too; at one workgroup a lane
    takes 8 or 9 (128 or 129) samples."""
    for c in (ec.CUBIC, ec.QUADRATIC):
        got = _one(native, integrator(c.expr, grid), c, rule, 0, c.at.n)
        want = ec.poly_value(c.coef, c.at, rule, 0, c.at.n)
        print(f"{c.name} grid {grid} {rule}: got {got!r} want {want!r}")
        assert got == want


@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("grid", [1, 3])
def test_expr_lane_split_edges_exact(native, integrator, grid, rule):
    """Slices from an odd sample whose lengths walk the edges of the balanced lane split:
    1, 3, 255 .. 257, the lane count and its neighbours, four per lane plus three."""
    for c, m in ec.edge_runs(grid):
        got = _one(native, integrator(c.expr, grid), c, rule, ec.EDGE_BEGIN, m)
        want = ec.poly_value(c.coef, c.at, rule, ec.EDGE_BEGIN, m)
        print(f"{c.name} grid {grid} {rule} n_local {m}: got {got!r} want {want!r}")
        assert got == want, (c.name, m)


@pytest.mark.parametrize("rule", ec.RULES)
def test_expr_full_lanes_exact(native, integrator, rule):
    """2048 workgroups with every lane at work: four samples each, five on the first three."""
    c = ec.FULL_LANES
    got = _one(native, integrator(c.expr, 2048), c, rule, 0, c.at.n)
    want = ec.poly_value(c.coef, c.at, rule, 0, c.at.n)
    print(f"{c.name} {rule}: got {got!r} want {want!r}")
    assert got == want


@pytest.mark.parametrize("grid", ec.EXPR_GRIDS)
def test_expr_rank_slices_exact(native, integrator, grid):
    """Seven rank slices, each against the reference of its own samples (five of them begin
    on odd samples), and with scale = 0.25."""
    c = ec.SLICE_CASE
    for r, (b, m) in enumerate(ec.rank_slices(c.at.n)):
        rule = ec.RULES[r % 3]
        got = _one(native, integrator(c.expr, grid), c, rule, b, m)
        want = ec.poly_value(c.coef, c.at, rule, b, m)
        print(f"rank {r} of {ec.WORLD} grid {grid} {rule}: got {got!r} want {want!r}")
        assert got == want, r
        assert _one(native, integrator(c.expr, grid), c, rule, b, m, 0.25) \
            == ec.poly_value(c.coef, c.at, rule, b, m, 0.25), r


@pytest.mark.parametrize("rule", ec.RULES)
def test_expr_scale_exact(native, integrator, rule):
    c = ec.CUBIC
    for grid in ec.EXPR_GRIDS:
        got = _one(native, integrator(c.expr, grid), c, rule, 0, c.at.n, 0.25)
        assert got == ec.poly_value(c.coef, c.at, rule, 0, c.at.n, 0.25), grid


def test_expr_loopback_ranks_exact(native, cuda):
    """Three loopback ranks, each its own slice of the cubic: the all-reduced value of every
    rank is the whole rule's reference."""
    c = ec.CUBIC
    for rule in ec.RULES:
        def body(rank, comm):
            ei = native.ExprIntegrator(c.expr, cuda.index, 3)
            b, m = ec.rank_slices(c.at.n, 3)[rank]
            return _one(native, ei, c, rule, b, m, 1.0, comm)
        out = loopback.run_ranks(3, body)
        want = ec.poly_value(c.coef, c.at, rule, 0, c.at.n)
        print(f"{rule}: ranks {out!r} want {want!r}")
        assert out == [want] * 3


def test_expr_per_lane_count_guard(native, integrator):
    """One workgroup and 2**40 samples: 2**32 per lane, one more than the kernel's 32-bit
    count holds. Refused before anything is launched; so is a begin + count that wraps."""
    ei = integrator(ec.CUBIC.expr, 1)
    n = 2**40
    with pytest.raises(RuntimeError, match="32-bit per-lane count"):
        ei.integrate(0.0, float(n), n, native.Rule.left, 0, n)
    with pytest.raises(RuntimeError, match="32-bit per-lane count"):
        ei.time(0.0, float(n), n, native.Rule.left, 0, n, 1)
    with pytest.raises(RuntimeError, match="slice outside"):
        ei.integrate(0.0, 1.0, 1000, native.Rule.left, 2**64 - 1, 2)
    with pytest.raises(RuntimeError, match="slice outside"):
        ei.time(0.0, 1.0, 1000, native.Rule.left, 2**64 - 1, 2, 1)
    # the object is as good as before
    c = ec.CUBIC
    assert _one(native, ei, c, "mid", 0, c.at.n) == ec.poly_value(c.coef, c.at, "mid", 0, c.at.n)


# ------------------------------------------------------------------------------ sweeps
def _sweep(expr, rows, at, rule, grid=0, begin=0, count=None) -> np.ndarray:
    v = kernels.riemann_expr_sweep(expr, np.asarray(rows, dtype=np.float64), at.a, at.b, at.n,
                                   rule=rule, grid=grid, i_begin=begin, n_local=count)
    return v.cpu().numpy()


@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("grid", ec.SWEEP_GRIDS)
def test_sweep_cubic_and_abs_rows_exact(cuda, grid, rule):
    """The unit vectors (the moments of the sample set, one by one), the cubic, a repeated
    row; and p2 + p1 |x - p0| with knots on and between samples: 1, 2, 7 sample slices and
    the auto shape."""
    at = ec.CUBIC.at
    _same(_sweep(ec.CUBIC_SWEEP, ec.CUBIC_ROWS, at, rule, grid),
          ec.poly_rows_values(ec.CUBIC_ROWS, at, rule, 0, at.n), f"cubic rows grid {grid} {rule}")
    _same(_sweep(ec.ABS_SWEEP, ec.abs_params(ec.ABS_ROWS, at.k), at, rule, grid),
          ec.abs_values(ec.ABS_ROWS, at, rule, 0, at.n), f"abs rows grid {grid} {rule}")


@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("grid,rows", list(ec.UNEQUAL_LANES))
def test_sweep_unequal_row_lanes_exact(native, cuda, grid, rows, rule):
    """Row lanes that walk four and three rows each (the alternating LDS slot over more than
    two rows, lanes that leave the loop at different times)."""
    at = ec.CUBIC.at
    assert native.expr_sweep_shape(at.n, rows, grid) == (grid, ec.UNEQUAL_LANES[grid, rows][0])
    r = ec.unequal_rows(rows)
    _same(_sweep(ec.CUBIC_SWEEP, r, at, rule, grid),
          ec.poly_rows_values(r.tolist(), at, rule, 0, at.n), f"{rows} rows grid {grid} {rule}")


@pytest.mark.parametrize("rule", ec.RULES)
@pytest.mark.parametrize("expr,rows", [(ec.HORNER8, ec.HORNER8_ROWS), (ec.HORNER5, ec.HORNER5_ROWS)],
                         ids=["8-parameters", "5-parameters"])
def test_sweep_wide_rows_exact(cuda, expr, rows, rule):
    """params[k * nparams + j] at 8 and 5 parameters: every row against its own reference, so
    a wrong stride shows as a wrong row."""
    at = ec.WIDE_AT
    for grid in (0, 2):
        _same(_sweep(expr, rows, at, rule, grid), ec.poly_rows_values(rows, at, rule, 0, at.n),
              f"{len(rows[0])} parameters grid {grid} {rule}")


@pytest.mark.parametrize("rule", ec.RULES)
def test_sweep_auto_shape_exact(native, cuda, rule):
    """1000 linear rows over 131 073 samples: the auto shape is 3 sample slices x 682 row
    lanes, some lanes take two rows and some one."""
    c = ec.AUTO_SHAPE
    assert native.expr_sweep_shape(c.at.n, c.rows) == ec.AUTO_SHAPE_GXGY
    _same(_sweep(ec.LINEAR_SWEEP, ec.linear_rows(c), c.at, rule), ec.linear_values(c, rule),
          f"{c.name} {rule}")


@pytest.mark.parametrize("rule", ec.RULES)
def test_sweep_row_chunks_exact(native, cuda, rule):
    """8195 rows at 2048 sample slices pass 2**24 partials: two chunks, 8192 rows and 3. All
    8195 values: the last three come from the second chunk, the first three must survive it."""
    c = ec.CHUNKED
    per = ec.chunk_rows(native, c)
    assert c.rows * c.grid > native.SWEEP_MAX_PARTIALS and per < c.rows <= 2 * per
    _same(_sweep(ec.LINEAR_SWEEP, ec.linear_rows(c), c.at, rule, c.grid),
          ec.linear_values(c, rule), f"{c.name} {rule}")


@pytest.mark.parametrize("rule", ec.RULES)
def test_sweep_samples_past_32_bits_exact(cuda, rule):
    c = ec.PAST_2_32
    b, m = c.at.span
    for grid in (0, 2):
        _same(_sweep(ec.LINEAR_SWEEP, ec.linear_rows(c), c.at, rule, grid, b, m),
              ec.linear_values(c, rule), f"{c.name} grid {grid} {rule}")


def test_sweep_rank_slices_exact(native, cuda):
    """Seven slices of the auto-shape case's first 50 rows and of the abs rows, each against
    the reference of its own samples; the right rule with scale = 0.25 through the object."""
    c = ec.AUTO_SHAPE
    rows = ec.linear_rows(c)[:50]
    for r, (b, m) in enumerate(ec.rank_slices(c.at.n)):
        rule = ec.RULES[r % 3]
        tot = ec.xr.exact_linear_rows_sums(rows, c.at.a_num, c.at.k, ec.OFF2[rule], b, m)
        _same(_sweep(ec.LINEAR_SWEEP, rows, c.at, rule, 0, b, m),
              ec.xr.values_f64(tot, c.at.k + 1) * 2.0 ** -c.at.k, f"linear rank {r} {rule}")
    at = ec.CUBIC.at
    es = native.ExprSweep(ec.ABS_SWEEP, 3, cuda.index, 2)
    params = np.asarray(ec.abs_params(ec.ABS_ROWS, at.k))
    for r, (b, m) in enumerate(ec.rank_slices(at.n)):
        got = es.integrate(params, at.a, at.b, at.n, native.Rule.right, b, m, 0.25)
        _same(got, ec.abs_values(ec.ABS_ROWS, at, "right", b, m, 0.25), f"abs rank {r} right")


@pytest.mark.parametrize("world", ec.LOOPBACK_WORLDS)
def test_sweep_loopback_ranks_exact(native, cuda, world):
    """W loopback ranks, each its own slice: every rank's all-reduced rows are the whole
    rule's references."""
    at = ec.CUBIC.at
    rows = np.asarray(ec.CUBIC_ROWS, dtype=np.float64)
    for rule in ec.RULES:
        def body(rank, comm):
            es = native.ExprSweep(ec.CUBIC_SWEEP, 4, cuda.index)
            b, m = ec.rank_slices(at.n, world)[rank]
            return es.integrate(rows, at.a, at.b, at.n, getattr(native.Rule, rule), b, m, 1.0,
                                comm)
        want = ec.poly_rows_values(ec.CUBIC_ROWS, at, rule, 0, at.n)
        for rank, v in enumerate(loopback.run_ranks(world, body)):
            _same(v, want, f"world {world} rank {rank} {rule}")


def test_sweep_object_reuse_exact(native, cuda):
    """One ExprSweep across 3 rows, then 700, then 5: the buffers grow and are kept; every
    value is the one a fresh object gives."""
    c = ec.AUTO_SHAPE
    es = native.ExprSweep(ec.LINEAR_SWEEP, 2, cuda.index)
    all_rows, want = ec.linear_rows(c), ec.linear_values(c, "mid")
    for k in ec.REUSE_ROWS:
        got = es.integrate(np.asarray(all_rows[:k], dtype=np.float64), c.at.a, c.at.b, c.at.n,
                           native.Rule.mid, 0, c.at.n)
        _same(got, want[:k], f"reuse {k} rows")


# ------------------------------------------------------------------------------ lifetime
@pytest.mark.parametrize("family", ["integrator", "sweep"])
def test_objects_own_their_loaded_module(native, cuda, family):
    """The cubic's 2085 samples, and three rows of its sweep, at grid 3."""
    c, at = ec.CUBIC, ec.CUBIC.at
    if family == "integrator":
        def make():
            return native.ExprIntegrator(c.expr, cuda.index, 3)

        def check(ei, what):
            want = ec.poly_value(c.coef, at, "mid", 0, at.n)
            assert _one(native, ei, c, "mid", 0, at.n) == want, what
    else:
        rows = ec.CUBIC_ROWS[3:6]

        def make():
            return native.ExprSweep(ec.CUBIC_SWEEP, 4, cuda.index, 3)

        def check(es, what):
            got = es.integrate(np.asarray(rows, dtype=np.float64), at.a, at.b, at.n,
                               native.Rule.mid, 0, at.n)
            _same(got, ec.poly_rows_values(rows, at, "mid", 0, at.n), what)
    ec.check_module_lifetime(make, check)
